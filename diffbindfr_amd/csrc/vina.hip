// Vina-function scoring and local minimisation of sampled poses (include/dbfr.h: dbfr_vina_*).
//
// The scoring function is the AutoDock Vina functional form (Trott & Olson, J. Comput. Chem. 2010) on a rigid receptor:
// five distance terms over heavy-atom pairs within 8 A, with the surface distance d = r - R_i - R_j; the full statement
// lives in diffbindfr_amd/vina.py and docs/vina.md.  One workgroup per pose (4 waves):
//   - the pose's receptor candidates (pocket atoms of the graph + the graph's optional extra atoms) within 8 A + margin of
//     the ligand are compacted, in atom order, into the pose's slice of the workspace; they are collected again only when
//     a ligand atom has moved by more than margin / 2 since the last collection (so no pair under 8 A is ever missed);
//   - ligand atoms are spread over the waves, a ligand atom's candidate pairs over the lanes; per-atom gradients are
//     reduced inside the wave (xor butterfly) and land in LDS, the energy terms are summed per lane in fp64 and reduced
//     wave by wave in a fixed order: no atomics, so a pose's result never depends on its batch mates;
//   - intra-ligand pairs are a symmetric bit matrix in LDS: each atom sums its own side of every pair.
// Minimisation: BFGS over (translation, rotation vector, torsions).  Positions are rebuilt from the starting conformation
// in the order of k_init_ligand (torsions in tor_bond order about the current bond axis, then the rotation about the
// centroid, then the translation), and the gradient with respect to those variables is exact: a reverse pass through the
// torsion sequence (the adjoint of each rotation, including the dependence of later axes on earlier torsions).
#include "common.h"

#define V_MAX_NL 256
#define V_MAX_TOR 58                  // 6 + 58 = 64 variables: the inverse Hessian (64 x 64 fp32) stays in LDS
#define V_MAX_VAR (6 + V_MAX_TOR)
#define V_THREADS 256
#define V_WAVES (V_THREADS / 64)
#define V_CUTOFF 8.0f
#define V_MAX_STEP 0.3f              // largest first-trial change of one variable (A or rad): keeps the minimisation in its basin
#define V_NTYPES 16                   // XS types 0..15; anything else is DUMMY

// XS type table: radius, hydrophobic, donor, acceptor
//                       C_H  C_P  N_P  N_D  N_A  N_DA O_P  O_D  O_A  O_DA S_P  P_P  F_H  Cl_H Br_H I_H
__constant__ float c_rad[V_NTYPES] = {1.9f, 1.9f, 1.8f, 1.8f, 1.8f, 1.8f, 1.7f, 1.7f, 1.7f, 1.7f, 2.0f, 2.1f, 1.5f, 1.8f, 2.0f, 2.2f};
__constant__ int c_flags[V_NTYPES] = {1, 0, 0, 2, 4, 6, 0, 2, 4, 6, 0, 0, 1, 1, 1, 1};   // 1 hydrophobic, 2 donor, 4 acceptor

#define W_GAUSS1 (-0.035579f)
#define W_GAUSS2 (-0.005156f)
#define W_REPULSION 0.840245f
#define W_HYDROPHOBIC (-0.035069f)
#define W_HBOND (-0.587439f)
#define W_NROT 0.05846f

struct VinaBatch {        // the fields of dbfr_batch / dbfr_vina_in the kernel reads (a slim kernel argument)
  const int32_t *lig_ptr, *bond_src, *bond_dst, *tor_ptr, *tor_bond, *atm_ptr;
  const float *lig_pos, *rec_pos;
  const uint8_t* rot_mask; const int64_t* rot_mask_off;
};
struct VinaIn {
  const int8_t *lig_type, *rec_type, *ext_type;
  const int32_t *pair_ptr, *pair_ij, *ext_ptr;
  const float* ext_pos;
};
struct VinaArgs {
  VinaIn in;
  VinaBatch b;
  float4* cand;            // [G * cap] candidate receptor atoms (x, y, z, type bits)
  int cap;                 // candidates per pose
  int max_iters; float grad_tol; float margin;
  int minimize;
  float* pos_out;          // [NL,3] or null
  float* terms;            // [G,8] or null
  float* grad_rigid;       // [G,6] or null
  float* grad_tor;         // [NTOR] or null
  int* iters;              // [G] or null
  const float* q_rigid;    // [G,6] starting variables (score at q) or null = 0
  const float* q_tor;      // [NTOR] or null = 0
};

struct VinaShared {
  float x0[3][V_MAX_NL];   // starting conformation
  float y[3][V_MAX_NL];    // after the torsions (before the rigid motion)
  float x[3][V_MAX_NL];    // current positions
  float g[3][V_MAX_NL];    // dE/dx, then the adjoint of y
  float xr[3][V_MAX_NL];   // positions at the last candidate collection
  uint32_t pm[V_MAX_NL][V_MAX_NL / 32];   // intra pairs, symmetric
  uint32_t tm[V_MAX_TOR][V_MAX_NL / 32];  // rot_node_mask rows
  int8_t lt[V_MAX_NL];
  int tu[V_MAX_TOR], tv[V_MAX_TOR];
  float tQ[V_MAX_TOR][9], tp[V_MAX_TOR][3], ta[V_MAX_TOR][3], tL[V_MAX_TOR];
  float H[V_MAX_VAR * V_MAX_VAR];
  float p[V_MAX_VAR], gp[V_MAX_VAR], d[V_MAX_VAR], pn[V_MAX_VAR], gn[V_MAX_VAR], hy[V_MAX_VAR];
  double red[V_WAVES][8];
  float rf[V_WAVES][8];
  float R[9], c[3], sc[8];
  double e[6];
  int ncand, flag;
};

__device__ __forceinline__ float wsum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wsumd(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// R = exp([v]x) (Rodrigues), row-major, applied as R x
__device__ void rotvec_to_mat(float vx, float vy, float vz, float* R) {
  float th = sqrtf(vx * vx + vy * vy + vz * vz);
  float s, c1;                       // sin(th)/th, (1-cos(th))/th^2
  if (th < 1e-4f) { s = 1.f - th * th / 6.f; c1 = 0.5f - th * th / 24.f; }
  else { s = sinf(th) / th; c1 = (1.f - cosf(th)) / (th * th); }
  R[0] = 1.f - c1 * (vy * vy + vz * vz); R[1] = -s * vz + c1 * vx * vy;         R[2] = s * vy + c1 * vx * vz;
  R[3] = s * vz + c1 * vx * vy;         R[4] = 1.f - c1 * (vx * vx + vz * vz); R[5] = -s * vx + c1 * vy * vz;
  R[6] = -s * vy + c1 * vx * vz;        R[7] = s * vx + c1 * vy * vz;         R[8] = 1.f - c1 * (vx * vx + vy * vy);
}

// Sum of v[0..5] over the block (fixed order: wave butterfly, then waves 0..3); every thread gets the result in out.
__device__ void block_sum6(VinaShared& S, const float* v, float* out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float r[6];
  for (int k = 0; k < 6; ++k) r[k] = wsum(v[k]);
  if (lane == 0)
    for (int k = 0; k < 6; ++k) S.rf[w][k] = r[k];
  __syncthreads();
  for (int k = 0; k < 6; ++k) {
    float s = 0.f;
    for (int q = 0; q < V_WAVES; ++q) s += S.rf[q][k];
    out[k] = s;
  }
  __syncthreads();
}

// One pair: the five unweighted inter terms' weighted sum split into e[0..4] and dE/dd.
__device__ __forceinline__ float pair_terms(int ti, int tj, float r, float* t5) {
  const float d = r - c_rad[ti] - c_rad[tj];
  const int fi = c_flags[ti], fj = c_flags[tj];
  const float q1 = d * 2.f;                              // d / 0.5
  const float g1 = expf(-q1 * q1);
  const float q2 = (d - 3.f) * 0.5f;
  const float g2 = expf(-q2 * q2);
  float de = W_GAUSS1 * g1 * (-2.f * q1 * 2.f) + W_GAUSS2 * g2 * (-2.f * q2 * 0.5f);
  t5[0] = W_GAUSS1 * g1;
  t5[1] = W_GAUSS2 * g2;
  t5[2] = 0.f; t5[3] = 0.f; t5[4] = 0.f;
  if (d < 0.f) { t5[2] = W_REPULSION * (d * d); de += W_REPULSION * 2.f * d; }
  if ((fi & 1) && (fj & 1)) {
    if (d < 0.5f) t5[3] = W_HYDROPHOBIC;
    else if (d < 1.5f) { t5[3] = W_HYDROPHOBIC * (1.5f - d); de -= W_HYDROPHOBIC; }
  }
  if (((fi & 2) && (fj & 4)) || ((fi & 4) && (fj & 2))) {
    if (d < -0.7f) t5[4] = W_HBOND;
    else if (d < 0.f) { t5[4] = W_HBOND * (-d / 0.7f); de -= W_HBOND / 0.7f; }
  }
  return de;
}

// Candidate collection: receptor atoms (pocket of graph g, then its extra atoms) within 8 A + margin of any ligand atom.
__device__ void collect(const VinaArgs& A, VinaShared& S, int g, int nl) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float4* out = A.cand + (size_t)g * A.cap;
  for (int i = tid; i < nl; i += V_THREADS) { S.xr[0][i] = S.x[0][i]; S.xr[1][i] = S.x[1][i]; S.xr[2][i] = S.x[2][i]; }
  const float lim = V_CUTOFF + A.margin, lim2 = lim * lim;
  const int a0 = A.b.atm_ptr[g], na = A.b.atm_ptr[g + 1] - a0;
  const int e0 = A.in.ext_ptr ? A.in.ext_ptr[g] : 0, ne = A.in.ext_ptr ? A.in.ext_ptr[g + 1] - e0 : 0;
  const int total = na + ne;
  int base = 0;
  if (tid == 0) S.ncand = 0;
  __syncthreads();
  for (int c0 = 0; c0 < total; c0 += V_THREADS) {
    const int c = c0 + tid;
    bool keep = false;
    float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < total) {
      const float* pp; int t;
      if (c < na) { pp = A.b.rec_pos + 3 * (size_t)(a0 + c); t = A.in.rec_type[a0 + c]; }
      else { pp = A.in.ext_pos + 3 * (size_t)(e0 + c - na); t = A.in.ext_type[e0 + c - na]; }
      if (t >= 0 && t < V_NTYPES) {
        rec = make_float4(pp[0], pp[1], pp[2], __int_as_float(t));
        for (int i = 0; i < nl && !keep; ++i) {
          float dx = rec.x - S.xr[0][i], dy = rec.y - S.xr[1][i], dz = rec.z - S.xr[2][i];
          keep = dx * dx + dy * dy + dz * dz < lim2;
        }
      }
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) S.rf[w][0] = __int_as_float(__popcll(m));
    __syncthreads();
    int off = base;
    for (int q = 0; q < w; ++q) off += __float_as_int(S.rf[q][0]);
    int cnt = base;
    for (int q = 0; q < V_WAVES; ++q) cnt += __float_as_int(S.rf[q][0]);
    if (keep) out[off + __popcll(m & ((1ull << lane) - 1ull))] = rec;
    base = cnt;
    __syncthreads();
  }
  if (tid == 0) S.ncand = base;
  __syncthreads();
}

// Energy terms into S.e[0..5] (five weighted inter terms, intra) and dE/dx into S.g.  Collects again when needed.
__device__ void evaluate(const VinaArgs& A, VinaShared& S, int g, int nl) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // has an atom moved by more than margin/2 since the last collection?
  int moved = 0;
  const float h2 = 0.25f * A.margin * A.margin;
  for (int i = tid; i < nl; i += V_THREADS) {
    float dx = S.x[0][i] - S.xr[0][i], dy = S.x[1][i] - S.xr[1][i], dz = S.x[2][i] - S.xr[2][i];
    moved |= dx * dx + dy * dy + dz * dz > h2;
  }
  if (__syncthreads_or(moved || S.flag)) {
    collect(A, S, g, nl);
    if (threadIdx.x == 0) S.flag = 0;
  }
  const float4* cand = A.cand + (size_t)g * A.cap;
  const int nc = S.ncand;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int i = w; i < nl; i += V_WAVES) {
    const int ti = S.lt[i];
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (ti >= 0 && ti < V_NTYPES) {
      const float xi = S.x[0][i], yi = S.x[1][i], zi = S.x[2][i];
      for (int c = lane; c < nc; c += 64) {
        const float4 r4 = cand[c];
        const float dx = xi - r4.x, dy = yi - r4.y, dz = zi - r4.z;
        const float r2 = dx * dx + dy * dy + dz * dz;
        if (r2 >= V_CUTOFF * V_CUTOFF) continue;
        const float r = sqrtf(r2);
        float t5[5];
        const float de = pair_terms(ti, __float_as_int(r4.w), r, t5);
        for (int k = 0; k < 5; ++k) acc[k] += (double)t5[k];
        const float f = r > 0.f ? de / r : 0.f;
        gx += f * dx; gy += f * dy; gz += f * dz;
      }
      for (int j = lane; j < nl; j += 64) {
        if (!((S.pm[i][j >> 5] >> (j & 31)) & 1u)) continue;
        const int tj = S.lt[j];
        if (tj < 0 || tj >= V_NTYPES) continue;
        const float dx = xi - S.x[0][j], dy = yi - S.x[1][j], dz = zi - S.x[2][j];
        const float r2 = dx * dx + dy * dy + dz * dz;
        if (r2 >= V_CUTOFF * V_CUTOFF) continue;
        const float r = sqrtf(r2);
        float t5[5];
        const float de = pair_terms(ti, tj, r, t5);
        if (j > i) acc[5] += (double)t5[0] + (double)t5[1] + (double)t5[2] + (double)t5[3] + (double)t5[4];
        const float f = r > 0.f ? de / r : 0.f;
        gx += f * dx; gy += f * dy; gz += f * dz;
      }
    }
    gx = wsum(gx); gy = wsum(gy); gz = wsum(gz);
    if (lane == 0) { S.g[0][i] = gx; S.g[1][i] = gy; S.g[2][i] = gz; }
  }
  for (int k = 0; k < 6; ++k) acc[k] = wsumd(acc[k]);
  if (lane == 0)
    for (int k = 0; k < 6; ++k) S.red[w][k] = acc[k];
  __syncthreads();
  if (tid < 6) {
    double s = 0.0;
    for (int q = 0; q < V_WAVES; ++q) s += S.red[q][tid];
    S.e[tid] = s;
  }
  __syncthreads();
}

// Positions from the variables q = (t[3], rotation vector[3], torsions[nt]): S.y (torsions applied to x0) and S.x.
__device__ void rebuild(VinaShared& S, const float* q, int nl, int nt) {
  const int tid = threadIdx.x;
  for (int i = tid; i < nl; i += V_THREADS) { S.y[0][i] = S.x0[0][i]; S.y[1][i] = S.x0[1][i]; S.y[2][i] = S.x0[2][i]; }
  __syncthreads();
  for (int k = 0; k < nt; ++k) {
    if (tid == 0) {
      const int u = S.tu[k], v = S.tv[k];
      float ax = S.y[0][u] - S.y[0][v], ay = S.y[1][u] - S.y[1][v], az = S.y[2][u] - S.y[2][v];
      const float L = sqrtf(ax * ax + ay * ay + az * az);
      ax /= L; ay /= L; az /= L;
      S.ta[k][0] = ax; S.ta[k][1] = ay; S.ta[k][2] = az; S.tL[k] = L;
      S.tp[k][0] = S.y[0][v]; S.tp[k][1] = S.y[1][v]; S.tp[k][2] = S.y[2][v];
      const float th = q[6 + k];
      rotvec_to_mat(ax * th, ay * th, az * th, S.tQ[k]);
    }
    __syncthreads();
    if (q[6 + k] != 0.f) {
      const float* Q = S.tQ[k];
      const float* p = S.tp[k];
      for (int i = tid; i < nl; i += V_THREADS)
        if ((S.tm[k][i >> 5] >> (i & 31)) & 1u) {
          const float x = S.y[0][i] - p[0], y = S.y[1][i] - p[1], z = S.y[2][i] - p[2];
          S.y[0][i] = (Q[0] * x + Q[1] * y + Q[2] * z) + p[0];
          S.y[1][i] = (Q[3] * x + Q[4] * y + Q[5] * z) + p[1];
          S.y[2][i] = (Q[6] * x + Q[7] * y + Q[8] * z) + p[2];
        }
      __syncthreads();
    }
  }
  if (tid < 3) {
    float s = 0.f;
    for (int i = 0; i < nl; ++i) s += S.y[tid][i];
    S.c[tid] = s / (float)nl;
  }
  if (tid == 0) rotvec_to_mat(q[3], q[4], q[5], S.R);
  __syncthreads();
  if (q[0] == 0.f && q[1] == 0.f && q[2] == 0.f && q[3] == 0.f && q[4] == 0.f && q[5] == 0.f) {   // no rigid motion: x = y exactly
    for (int i = tid; i < nl; i += V_THREADS) { S.x[0][i] = S.y[0][i]; S.x[1][i] = S.y[1][i]; S.x[2][i] = S.y[2][i]; }
    __syncthreads();
    return;
  }
  for (int i = tid; i < nl; i += V_THREADS) {   // R (y - c) + c + t
    const float x = S.y[0][i] - S.c[0], y = S.y[1][i] - S.c[1], z = S.y[2][i] - S.c[2];
    S.x[0][i] = (S.R[0] * x + S.R[1] * y + S.R[2] * z) + S.c[0] + q[0];
    S.x[1][i] = (S.R[3] * x + S.R[4] * y + S.R[5] * z) + S.c[1] + q[1];
    S.x[2][i] = (S.R[6] * x + S.R[7] * y + S.R[8] * z) + S.c[2] + q[2];
  }
  __syncthreads();
}

// Gradient with respect to q from S.g = dE/dx (consumes S.g and S.y).  At q = 0 this is the generalised gradient.
__device__ void param_grad(VinaShared& S, const float* q, float* gq, int nl, int nt) {
  const int tid = threadIdx.x;
  float v[6] = {0, 0, 0, 0, 0, 0}, s6[6];
  if (tid < nl) {
    const float gx = S.g[0][tid], gy = S.g[1][tid], gz = S.g[2][tid];
    const float rx = S.x[0][tid] - S.c[0] - q[0], ry = S.x[1][tid] - S.c[1] - q[1], rz = S.x[2][tid] - S.c[2] - q[2];
    v[0] = gx; v[1] = gy; v[2] = gz;
    v[3] = ry * gz - rz * gy; v[4] = rz * gx - rx * gz; v[5] = rx * gy - ry * gx;
  }
  block_sum6(S, v, s6);
  if (tid == 0) {
    gq[0] = s6[0]; gq[1] = s6[1]; gq[2] = s6[2];
    // g_w = J_l(w)^T tau = tau - A w x tau + B w x (w x tau)
    const float wx = q[3], wy = q[4], wz = q[5];
    const float th2 = wx * wx + wy * wy + wz * wz, th = sqrtf(th2);
    float Ac, Bc;
    if (th < 1e-3f) { Ac = 0.5f - th2 / 24.f; Bc = 1.f / 6.f - th2 / 120.f; }
    else { Ac = (1.f - cosf(th)) / th2; Bc = (th - sinf(th)) / (th2 * th); }
    const float tx = s6[3], ty = s6[4], tz = s6[5];
    const float cx = wy * tz - wz * ty, cy = wz * tx - wx * tz, cz = wx * ty - wy * tx;
    const float ccx = wy * cz - wz * cy, ccy = wz * cx - wx * cz, ccz = wx * cy - wy * cx;
    gq[3] = tx - Ac * cx + Bc * ccx; gq[4] = ty - Ac * cy + Bc * ccy; gq[5] = tz - Ac * cz + Bc * ccz;
    S.sc[0] = s6[0]; S.sc[1] = s6[1]; S.sc[2] = s6[2];
  }
  if (nt == 0) { __syncthreads(); return; }
  __syncthreads();
  // adjoint of y: ybar_i = R^T g_i + (1/n)(I - R^T) G
  const float inv_n = 1.f / (float)nl;
  for (int i = tid; i < nl; i += V_THREADS) {
    const float gx = S.g[0][i], gy = S.g[1][i], gz = S.g[2][i];
    const float Gx = S.sc[0], Gy = S.sc[1], Gz = S.sc[2];
    const float* R = S.R;
    const float RtG0 = R[0] * Gx + R[3] * Gy + R[6] * Gz, RtG1 = R[1] * Gx + R[4] * Gy + R[7] * Gz, RtG2 = R[2] * Gx + R[5] * Gy + R[8] * Gz;
    S.g[0][i] = (R[0] * gx + R[3] * gy + R[6] * gz) + (Gx - RtG0) * inv_n;
    S.g[1][i] = (R[1] * gx + R[4] * gy + R[7] * gz) + (Gy - RtG1) * inv_n;
    S.g[2][i] = (R[2] * gx + R[5] * gy + R[8] * gz) + (Gz - RtG2) * inv_n;
  }
  __syncthreads();
  for (int k = nt - 1; k >= 0; --k) {
    const float* p = S.tp[k];
    const bool in = tid < nl && ((S.tm[k][tid >> 5] >> (tid & 31)) & 1u);
    float t6[6] = {0, 0, 0, 0, 0, 0};
    if (in) {
      const float bx = S.g[0][tid], by = S.g[1][tid], bz = S.g[2][tid];
      const float rx = S.y[0][tid] - p[0], ry = S.y[1][tid] - p[1], rz = S.y[2][tid] - p[2];
      t6[0] = ry * bz - rz * by; t6[1] = rz * bx - rx * bz; t6[2] = rx * by - ry * bx;
      t6[3] = bx; t6[4] = by; t6[5] = bz;
    }
    block_sum6(S, t6, s6);
    const float* a = S.ta[k];
    const float th = q[6 + k];
    if (tid == 0) gq[6 + k] = a[0] * s6[0] + a[1] * s6[1] + a[2] * s6[2];
    if (th != 0.f) {
      const float* Q = S.tQ[k];
      if (in) {   // ybar <- Q^T ybar, y <- Q^T (y - p) + p
        const float bx = S.g[0][tid], by = S.g[1][tid], bz = S.g[2][tid];
        S.g[0][tid] = Q[0] * bx + Q[3] * by + Q[6] * bz;
        S.g[1][tid] = Q[1] * bx + Q[4] * by + Q[7] * bz;
        S.g[2][tid] = Q[2] * bx + Q[5] * by + Q[8] * bz;
        const float x = S.y[0][tid] - p[0], y = S.y[1][tid] - p[1], z = S.y[2][tid] - p[2];
        S.y[0][tid] = (Q[0] * x + Q[3] * y + Q[6] * z) + p[0];
        S.y[1][tid] = (Q[1] * x + Q[4] * y + Q[7] * z) + p[1];
        S.y[2][tid] = (Q[2] * x + Q[5] * y + Q[8] * z) + p[2];
      }
      __syncthreads();
      if (tid == 0) {
        // the axis moves with its atoms: dQ Q^T = [sin(th) da + (1 - cos(th)) a x da]x, da = (I - a a^T)(dy_u - dy_v) / L
        const float tx = s6[0], ty = s6[1], tz = s6[2];
        const float sn = sinf(th), cs1 = 1.f - cosf(th);
        const float wx = sn * tx + cs1 * (ty * a[2] - tz * a[1]);
        const float wy = sn * ty + cs1 * (tz * a[0] - tx * a[2]);
        const float wz = sn * tz + cs1 * (tx * a[1] - ty * a[0]);
        const float aw = a[0] * wx + a[1] * wy + a[2] * wz;
        const float invL = 1.f / S.tL[k];
        const float gA[3] = {(wx - a[0] * aw) * invL, (wy - a[1] * aw) * invL, (wz - a[2] * aw) * invL};
        // pivot: (I - Q)^T F
        const float Fx = s6[3], Fy = s6[4], Fz = s6[5];
        const float pv[3] = {Fx - (Q[0] * Fx + Q[3] * Fy + Q[6] * Fz), Fy - (Q[1] * Fx + Q[4] * Fy + Q[7] * Fz),
                             Fz - (Q[2] * Fx + Q[5] * Fy + Q[8] * Fz)};
        const int u = S.tu[k], v = S.tv[k];
        for (int c = 0; c < 3; ++c) { S.g[c][u] += gA[c]; S.g[c][v] += pv[c] - gA[c]; }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(V_THREADS) void k_vina(VinaArgs A) {
  __shared__ VinaShared S;
  const int g = blockIdx.x, tid = threadIdx.x;
  const VinaBatch& b = A.b;
  const int l0 = b.lig_ptr[g], nl = b.lig_ptr[g + 1] - l0;
  const int k0 = b.tor_ptr[g], nt = b.tor_ptr[g + 1] - k0;
  const int n = 6 + nt;
  const int na = b.atm_ptr[g + 1] - b.atm_ptr[g], ne = A.in.ext_ptr ? A.in.ext_ptr[g + 1] - A.in.ext_ptr[g] : 0;
  if (nl <= 0 || nl > V_MAX_NL || nt < 0 || nt > V_MAX_TOR || na < 0 || ne < 0 || na + ne > A.cap) {
    // the host-side maxima (max_nl, max_tor, max_na, max_ext) understated this graph: NaN results, nothing touched
    if (tid < 8 && A.terms) A.terms[8 * (size_t)g + tid] = __int_as_float(0x7fc00000);
    if (tid == 0 && A.iters) A.iters[g] = -1;
    return;
  }
  for (int i = tid; i < nl; i += V_THREADS) {
    for (int c = 0; c < 3; ++c) S.x0[c][i] = S.x[c][i] = S.xr[c][i] = b.lig_pos[3 * (size_t)(l0 + i) + c];
    S.lt[i] = A.in.lig_type[l0 + i];
  }
  for (int i = tid; i < V_MAX_NL * (V_MAX_NL / 32); i += V_THREADS) (&S.pm[0][0])[i] = 0u;
  for (int i = tid; i < nt * (V_MAX_NL / 32); i += V_THREADS) (&S.tm[0][0])[i] = 0u;
  __syncthreads();
  const int p0 = A.in.pair_ptr[g], np = A.in.pair_ptr[g + 1] - p0;
  for (int k = tid; k < np; k += V_THREADS) {
    const int i = A.in.pair_ij[2 * (size_t)(p0 + k)] - l0, j = A.in.pair_ij[2 * (size_t)(p0 + k) + 1] - l0;
    if (i < 0 || i >= nl || j < 0 || j >= nl) continue;
    atomicOr(&S.pm[i][j >> 5], 1u << (j & 31));   // integer bit sets: order-free
    atomicOr(&S.pm[j][i >> 5], 1u << (i & 31));
  }
  for (int k = 0; k < nt; ++k) {
    const uint8_t* m = b.rot_mask + b.rot_mask_off[k0 + k];
    for (int i = tid; i < nl; i += V_THREADS)
      if (m[i]) atomicOr(&S.tm[k][i >> 5], 1u << (i & 31));
  }
  int bad = 0;
  if (tid < nt) {
    const int e = b.tor_bond[k0 + tid];
    const int u = b.bond_src[e] - l0, v = b.bond_dst[e] - l0;
    bad = u < 0 || u >= nl || v < 0 || v >= nl || u == v;
    S.tu[tid] = bad ? 0 : u; S.tv[tid] = bad ? 0 : v;
  }
  if (__syncthreads_or(bad)) {   // a torsion bond outside the graph's atoms: NaN results, nothing touched
    if (tid < 8 && A.terms) A.terms[8 * (size_t)g + tid] = __int_as_float(0x7fc00000);
    if (tid == 0 && A.iters) A.iters[g] = -1;
    return;
  }
  for (int k = tid; k < V_MAX_VAR; k += V_THREADS) {
    S.p[k] = 0.f;
    S.pn[k] = k < 6 ? (A.q_rigid ? A.q_rigid[6 * (size_t)g + k] : 0.f) : (k < n && A.q_tor ? A.q_tor[k0 + k - 6] : 0.f);
  }
  for (int i = tid; i < n * n; i += V_THREADS) S.H[i] = (i / n == i % n) ? 1.f : 0.f;
  if (tid == 0) S.flag = 1;   // collect the candidates at the first evaluation
  __syncthreads();
  // One evaluation per pass (a single call site of rebuild / evaluate / param_grad each keeps the scalar registers in
  // budget): phase 0 = the start q = 0, 1 = a line-search trial at pn = p + alpha d, 2 = back to p after a stalled search.
  int phase = 0, it = 0, ls = 0;
  bool identity = true;
  double f = 0.0;
  float alpha = 0.f, slope = 0.f;
  for (;;) {
    rebuild(S, S.pn, nl, nt);
    evaluate(A, S, g, nl);
    const double fn = S.e[0] + S.e[1] + S.e[2] + S.e[3] + S.e[4] + S.e[5];
    if (phase == 2) break;
    bool take = phase == 0, redirect = false;
    if (phase == 1) {
      if (fn <= f + 1e-4 * (double)alpha * (double)slope) take = true;   // Armijo
      else if (++ls < 24) {
        alpha *= 0.5f;
        if (tid < n) S.pn[tid] = S.p[tid] + alpha * S.d[tid];
        __syncthreads();
        continue;
      } else if (!identity) {   // the quasi-Newton direction failed: start again from steepest descent
        for (int i = tid; i < n * n; i += V_THREADS) S.H[i] = (i / n == i % n) ? 1.f : 0.f;
        identity = true;
        redirect = true;
        __syncthreads();
      } else {                  // not even steepest descent lowers the objective: its resolution is reached
        if (tid < n) S.pn[tid] = S.p[tid];
        phase = 2;
        __syncthreads();
        continue;
      }
    }
    if (take) {
      param_grad(S, S.pn, S.gn, nl, nt);
      __syncthreads();
      if (phase == 1) {
        // BFGS update of the inverse Hessian with s = pn - p, y = gn - g (skipped unless s.y > 0)
        float sy = 0.f;
        for (int k = 0; k < n; ++k) sy += (S.pn[k] - S.p[k]) * (S.gn[k] - S.gp[k]);
        if (sy > 0.f) {
          if (tid < n) {
            float s = 0.f;
            for (int k = 0; k < n; ++k) s += S.H[tid * n + k] * (S.gn[k] - S.gp[k]);
            S.hy[tid] = s;
          }
          __syncthreads();
          float yhy = 0.f;
          for (int k = 0; k < n; ++k) yhy += (S.gn[k] - S.gp[k]) * S.hy[k];
          const float r = 1.f / sy, c = (1.f + yhy * r) * r;
          for (int idx = tid; idx < n * n; idx += V_THREADS) {
            const int i = idx / n, j = idx % n;
            const float si = S.pn[i] - S.p[i], sj = S.pn[j] - S.p[j];
            S.H[idx] += c * si * sj - r * (S.hy[i] * sj + si * S.hy[j]);
          }
          identity = false;
        }
        ++it;
      }
      __syncthreads();
      if (tid < n) { S.p[tid] = S.pn[tid]; S.gp[tid] = S.gn[tid]; }
      f = fn;
      __syncthreads();
    }
    if (!A.minimize) break;
    float gmax = 0.f;
    for (int k = 0; k < n; ++k) gmax = fmaxf(gmax, fabsf(S.gp[k]));
    if (gmax < A.grad_tol || it >= A.max_iters) {
      if (!redirect) break;     // the positions in S.x are those of p
      if (tid < n) S.pn[tid] = S.p[tid];
      phase = 2;
      __syncthreads();
      continue;
    }
    if (tid < n) {             // d = -H g
      float s = 0.f;
      for (int k = 0; k < n; ++k) s += S.H[tid * n + k] * S.gp[k];
      S.d[tid] = -s;
    }
    __syncthreads();
    float dmax = 0.f;
    slope = 0.f;
    for (int k = 0; k < n; ++k) { slope += S.gp[k] * S.d[k]; dmax = fmaxf(dmax, fabsf(S.d[k])); }
    if (!(slope < 0.f)) {       // not a descent direction: steepest descent from a fresh Hessian
      __syncthreads();
      if (tid < n) S.d[tid] = -S.gp[tid];
      for (int i = tid; i < n * n; i += V_THREADS) S.H[i] = (i / n == i % n) ? 1.f : 0.f;
      identity = true;
      __syncthreads();
      slope = 0.f; dmax = 0.f;
      for (int k = 0; k < n; ++k) { slope += S.gp[k] * S.d[k]; dmax = fmaxf(dmax, fabsf(S.d[k])); }
    }
    alpha = fminf(1.f, V_MAX_STEP / dmax);   // a local search: no variable moves by more than V_MAX_STEP in a first trial
    ls = 0;
    phase = 1;
    if (tid < n) S.pn[tid] = S.p[tid] + alpha * S.d[tid];
    __syncthreads();
  }
  if (tid == 0) {
    if (A.terms) {
      float* t = A.terms + 8 * (size_t)g;
      double inter = 0.0;
      for (int k = 0; k < 5; ++k) { t[k] = (float)S.e[k]; inter += S.e[k]; }
      t[5] = (float)S.e[5];
      t[6] = (float)(inter + S.e[5]);
      t[7] = (float)(inter / (1.0 + (double)W_NROT * nt));
    }
    if (A.iters) A.iters[g] = it;
  }
  if (!A.minimize) {
    if (A.grad_rigid && tid < 6) A.grad_rigid[6 * (size_t)g + tid] = S.gp[tid];
    if (A.grad_tor && tid < nt) A.grad_tor[k0 + tid] = S.gp[6 + tid];
  }
  if (A.pos_out)
    for (int i = tid; i < nl; i += V_THREADS)
      for (int c = 0; c < 3; ++c) A.pos_out[3 * (size_t)(l0 + i) + c] = S.x[c][i];
}

// ------------------------------------------------------------------------------------------------ C ABI
static int vina_check(const dbfr_vina_in* in, size_t* cap_per_pose) {
  if (!in || !in->batch) { dbfr_set_error("dbfr_vina: null argument"); return DBFR_ERR_ARG; }
  const dbfr_batch* b = in->batch;
  if (b->G <= 0 || b->NL <= 0) { dbfr_set_error("dbfr_vina: empty batch"); return DBFR_ERR_ARG; }
  if (b->max_nl <= 0 || b->max_nl > V_MAX_NL) {
    dbfr_set_error("dbfr_vina: ligand with more than 256 heavy atoms is not supported (max_nl must be in 1..256)");
    return DBFR_ERR_ARG;
  }
  if (in->max_tor < 0 || in->max_tor > V_MAX_TOR) {
    dbfr_set_error("dbfr_vina: ligand with more than 58 torsions is not supported (max_tor must be in 0..58)");
    return DBFR_ERR_ARG;
  }
  if (b->max_na < 0 || b->max_na > 8192) {
    dbfr_set_error("dbfr_vina: pocket with more than 8192 heavy atoms is not supported");
    return DBFR_ERR_ARG;
  }
  if (in->ext_ptr && (in->max_ext < 0 || !in->ext_pos || !in->ext_type)) {
    dbfr_set_error("dbfr_vina: ext_ptr needs ext_pos, ext_type and max_ext >= 0");
    return DBFR_ERR_ARG;
  }
  if (!b->lig_ptr || !b->lig_pos || !b->atm_ptr || !b->rec_pos || !b->tor_ptr || (b->NTOR > 0 && (!b->tor_bond || !b->rot_mask ||
      !b->rot_mask_off || !b->bond_src || !b->bond_dst)) || !in->lig_type || !in->rec_type || !in->pair_ptr ||
      (!in->pair_ij && in->n_pairs > 0)) {
    dbfr_set_error("dbfr_vina: null device pointer in the input");
    return DBFR_ERR_ARG;
  }
  size_t cap = (size_t)b->max_na + (in->ext_ptr ? (size_t)in->max_ext : 0);
  if (cap < 1) cap = 1;
  *cap_per_pose = cap;
  return DBFR_OK;
}

extern "C" int dbfr_vina_workspace_bytes(const dbfr_vina_in* in, size_t* bytes) {
  size_t cap;
  int rc = vina_check(in, &cap);
  if (rc) return rc;
  if (!bytes) { dbfr_set_error("dbfr_vina_workspace_bytes: null argument"); return DBFR_ERR_ARG; }
  *bytes = (size_t)in->batch->G * cap * sizeof(float4);
  return DBFR_OK;
}

static int vina_launch(const dbfr_vina_in* in, int minimize, const dbfr_vina_opts* opts, const float* q_rigid, const float* q_tor,
                       float* pos_out, float* terms, float* grad_rigid, float* grad_tor, int32_t* iters, void* ws, size_t ws_bytes,
                       void* stream) {
  size_t cap;
  int rc = vina_check(in, &cap);
  if (rc) return rc;
  const size_t need = (size_t)in->batch->G * cap * sizeof(float4);
  if (!ws || ws_bytes < need) {
    dbfr_set_error("dbfr_vina: workspace of " + std::to_string(ws_bytes) + " bytes, this batch needs " + std::to_string(need) +
                   " (dbfr_vina_workspace_bytes)");
    return DBFR_ERR_ARG;
  }
  VinaArgs A;
  memset(&A, 0, sizeof A);
  const dbfr_batch* B = in->batch;
  A.b = {B->lig_ptr, B->bond_src, B->bond_dst, B->tor_ptr, B->tor_bond, B->atm_ptr, B->lig_pos, B->rec_pos, B->rot_mask, B->rot_mask_off};
  A.in = {in->lig_type, in->rec_type, in->ext_type, in->pair_ptr, in->pair_ij, in->ext_ptr, in->ext_pos};
  A.cand = (float4*)ws;
  A.cap = (int)cap;
  A.max_iters = 100; A.grad_tol = 1e-3f; A.margin = 2.f;
  if (opts) {
    if (opts->max_iters < 0 || !(opts->grad_tol >= 0.f) || !(opts->margin > 0.f)) {
      dbfr_set_error("dbfr_vina_minimize: max_iters >= 0, grad_tol >= 0 and margin > 0 required");
      return DBFR_ERR_ARG;
    }
    A.max_iters = opts->max_iters; A.grad_tol = opts->grad_tol; A.margin = opts->margin;
  }
  A.minimize = minimize;
  A.q_rigid = q_rigid; A.q_tor = in->batch->NTOR > 0 ? q_tor : nullptr;
  A.pos_out = pos_out; A.terms = terms; A.grad_rigid = grad_rigid; A.grad_tor = grad_tor; A.iters = iters;
  hipLaunchKernelGGL(k_vina, dim3(in->batch->G), dim3(V_THREADS), 0, (hipStream_t)stream, A);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

extern "C" int dbfr_vina_score(const dbfr_vina_in* in, float* terms, float* grad_rigid, float* grad_tor, void* workspace,
                               size_t workspace_bytes, void* hip_stream) {
  return vina_launch(in, 0, nullptr, nullptr, nullptr, nullptr, terms, grad_rigid, grad_tor, nullptr, workspace, workspace_bytes,
                     hip_stream);
}

extern "C" int dbfr_vina_score_at(const dbfr_vina_in* in, const float* q_rigid, const float* q_tor, float* lig_pos_out, float* terms,
                                  float* grad_rigid, float* grad_tor, void* workspace, size_t workspace_bytes, void* hip_stream) {
  return vina_launch(in, 0, nullptr, q_rigid, q_tor, lig_pos_out, terms, grad_rigid, grad_tor, nullptr, workspace, workspace_bytes,
                     hip_stream);
}

extern "C" int dbfr_vina_minimize(const dbfr_vina_in* in, const dbfr_vina_opts* opts, float* lig_pos_out, float* terms,
                                  int32_t* iters, void* workspace, size_t workspace_bytes, void* hip_stream) {
  return vina_launch(in, 1, opts, nullptr, nullptr, lig_pos_out, terms, nullptr, nullptr, iters, workspace, workspace_bytes, hip_stream);
}
