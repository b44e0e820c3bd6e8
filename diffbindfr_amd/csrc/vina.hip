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
//
// Flexible pocket side chains (dbfr_vina_flex_*): the same device functions, instantiated a second time with larger capacities
// (VinaShared<V_FLEX_MAX_TOR>, dynamic LDS).  The pose's flexible receptor atoms become movable slots nl .. nl + nf - 1 behind the
// ligand's, every fixed end of a flexible torsion's axis (CA, CB) a DUMMY-typed anchor slot behind those that nothing moves; the
// flexible torsions follow the ligand's in q.  The pair matrix carries ligand-flexible pairs (E_inter) and the allowed
// flexible-flexible pairs (E_rec); flexible atoms are left out of the candidate list, and a candidate carries its receptor index
// so that a flexible atom skips the partners on its exclusion list.  Nothing here knows an amino acid: diffbindfr_amd/vina_flex.py
// (flex_topology) turns residues into these lists.  Everything flexible sits behind `if constexpr (SH::kFlex)`: the rigid
// instantiation keeps its LDS, its occupancy and, bit for bit, its results (its register allocation moved a little:
// profiles/r17_vinaflex_resource_usage.txt).
//
// Monte-Carlo search (dbfr_vina_search, k_vina_search): Vina's iterated local search around the same minimiser, one workgroup per
// (pose, chain).  vina_pose is split for it into vina_setup (the graph into LDS), vina_bfgs (the BFGS loop) and the outputs; the
// search's LDS struct is the rigid one plus the best pose and the box.  Its random numbers are counter-based (Philox4x32-10), and
// the generator and the mutation are __host__ __device__ so that the host tests them (dbfr_test_philox4x32, dbfr_test_vina_mutation).
// k_vina_search is a template over the LDS struct as k_vina is: k_vina_search<V_MAX_TOR> is that rigid search, and
// k_vina_search<V_FLEX_MAX_TOR> (dbfr_vina_flex_search; docs/vina.md, "Search with flexible side chains") runs the same stages over
// the flexible minimiser's variables: the base of `rebuild` and the best pose cover all slots, a step may redraw a flexible torsion,
// and two accumulators per flexible torsion keep the angles that re-basing would forget.
#include "common.h"
#define VINA_XS_RAD c_rad
#define VINA_XS_FLAGS c_flags
#include "vina_terms.h"
#include <algorithm>

#define V_MAX_NL 256
#define V_MAX_TOR 58                  // 6 + 58 = 64 variables: the inverse Hessian (64 x 64 fp32) stays in LDS
#define V_FLEX_MAX_TOR 122            // the flexible instantiation: 6 + 122 = 128 variables, a 64 KB inverse Hessian in dynamic LDS
#define V_FLEX_MAX_EXCL 32            // receptor atoms within 3 bonds of a flexible atom (pocketcheck's limit)
#define V_FLEX_MAX_NA 8192            // pocket atoms of a pose (the flexible-atom bit set)
#define V_THREADS 256
#define V_WAVES (V_THREADS / 64)
#define V_MAX_STEP 0.3f              // largest first-trial change of one variable (A or rad): keeps the minimisation in its basin

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
  // flexible instantiation only (dbfr_vina_flex_in and the flexible outputs)
  const int32_t *f_ptr, *f_atom, *ft_ptr, *ft_bc, *turn_ptr, *turn, *excl_ptr, *excl;
  const float* q_flex;     // [NFT] or null = 0
  float *rec_out, *q_flex_out, *grad_flex;
};

template <bool F> struct VinaFlexShared {};
template <> struct VinaFlexShared<true> {
  uint32_t fm[V_FLEX_MAX_NA / 32];   // the pocket atoms that are flexible in this pose
  int fa[V_MAX_NL];                  // pocket index of flexible atom r (slot nl + r)
};
template <int MT> struct VinaShared : VinaFlexShared<(MT > V_MAX_TOR)> {
  static constexpr bool kFlex = MT > V_MAX_TOR;
  static constexpr int kMaxVar = 6 + MT;
  float x0[3][V_MAX_NL];   // starting conformation
  float y[3][V_MAX_NL];    // after the torsions (before the rigid motion)
  float x[3][V_MAX_NL];    // current positions
  float g[3][V_MAX_NL];    // dE/dx, then the adjoint of y
  float xr[3][V_MAX_NL];   // positions at the last candidate collection
  uint32_t pm[V_MAX_NL][V_MAX_NL / 32];   // intra pairs, symmetric
  uint32_t tm[MT][V_MAX_NL / 32];         // rot_node_mask rows
  int8_t lt[V_MAX_NL];
  int tu[MT], tv[MT];
  float tQ[MT][9], tp[MT][3], ta[MT][3], tL[MT];
  float H[kMaxVar * kMaxVar];
  float p[kMaxVar], gp[kMaxVar], d[kMaxVar], pn[kMaxVar], gn[kMaxVar], hy[kMaxVar];
  double red[V_WAVES][8];
  float rf[V_WAVES][8];
  float R[9], c[3], sc[8];
  double e[kFlex ? 8 : 6];  // five inter terms, intra (, E_rec)
  int ncand, flag;
};
static_assert(sizeof(VinaShared<V_MAX_TOR>) == 48280, "the rigid instantiation's LDS struct (and with it k_vina's occupancy) must not change");
static_assert(sizeof(VinaShared<V_FLEX_MAX_TOR>) <= 160 * 1024 - 64, "the flexible instantiation must fit the gfx950 workgroup LDS limit");

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
template <class SH> __device__ void block_sum6(SH& S, const float* v, float* out) {
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

// Candidate collection: fixed receptor atoms (pocket of graph g, then its extra atoms) within 8 A + margin of any of the ns slots
// (the ligand atoms; with flexible side chains also their atoms, which are no candidates themselves).
template <class SH> __device__ void collect(const VinaArgs& A, SH& S, int g, int ns) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float4* out = A.cand + (size_t)g * A.cap;
  for (int i = tid; i < ns; i += V_THREADS) { S.xr[0][i] = S.x[0][i]; S.xr[1][i] = S.x[1][i]; S.xr[2][i] = S.x[2][i]; }
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
      const bool typed = v_typed(t);
      bool fixed = true;
      if constexpr (SH::kFlex) {   // flexible atoms are slots, not candidates; a candidate carries its receptor index above its type
        fixed = c >= na || !((S.fm[c >> 5] >> (c & 31)) & 1u);
        t |= c << 5;
      }
      if (typed && fixed) {
        rec = make_float4(pp[0], pp[1], pp[2], __int_as_float(t));
        for (int i = 0; i < ns && !keep; ++i) {
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
// Flexible: slots nl .. ns - 1 are receptor atoms; S.e[6] = E_rec (flexible-fixed pairs off the exclusion list, allowed
// flexible-flexible pairs); a ligand-flexible pair counts in the inter terms, from the ligand atom's side.
template <class SH> __device__ void evaluate(const VinaArgs& A, SH& S, int g, int nl, int ns) {
  constexpr int NE = SH::kFlex ? 7 : 6;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // has an atom moved by more than margin/2 since the last collection?
  int moved = 0;
  const float h2 = 0.25f * A.margin * A.margin;
  for (int i = tid; i < ns; i += V_THREADS) {
    float dx = S.x[0][i] - S.xr[0][i], dy = S.x[1][i] - S.xr[1][i], dz = S.x[2][i] - S.xr[2][i];
    moved |= dx * dx + dy * dy + dz * dz > h2;
  }
  if (__syncthreads_or(moved || S.flag)) {
    collect(A, S, g, ns);
    if (threadIdx.x == 0) S.flag = 0;
  }
  const float4* cand = A.cand + (size_t)g * A.cap;
  const int nc = S.ncand;
  double acc[NE];
  for (int k = 0; k < NE; ++k) acc[k] = 0.0;
  for (int i = w; i < ns; i += V_WAVES) {
    const int ti = S.lt[i];
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (v_typed(ti)) {
      const float xi = S.x[0][i], yi = S.x[1][i], zi = S.x[2][i];
      int ex0 = 0, ex1 = 0;        // a flexible atom's exclusion list (wave-uniform)
      if constexpr (SH::kFlex)
        if (i >= nl) { const int f = A.f_ptr[g] + i - nl; ex0 = A.excl_ptr[f]; ex1 = A.excl_ptr[f + 1]; }
      for (int c = lane; c < nc; c += 64) {
        const float4 r4 = cand[c];
        const float dx = xi - r4.x, dy = yi - r4.y, dz = zi - r4.z;
        const float r2 = dx * dx + dy * dy + dz * dz;
        if (r2 >= V_CUTOFF * V_CUTOFF) continue;
        int tj = __float_as_int(r4.w);
        if constexpr (SH::kFlex) {
          const int rj = tj >> 5;
          tj &= 31;
          bool skip = false;
          for (int k = ex0; k < ex1; ++k) skip |= A.excl[k] == rj;
          if (skip) continue;
        }
        const float r = sqrtf(r2);
        float t5[5];
        const float de = pair_terms<true>(ti, tj, r, t5);
        if (SH::kFlex && i >= nl) acc[NE - 1] += (double)t5[0] + (double)t5[1] + (double)t5[2] + (double)t5[3] + (double)t5[4];
        else for (int k = 0; k < 5; ++k) acc[k] += (double)t5[k];
        const float f = r > 0.f ? de / r : 0.f;
        gx += f * dx; gy += f * dy; gz += f * dz;
      }
      for (int j = lane; j < ns; j += 64) {
        if (!((S.pm[i][j >> 5] >> (j & 31)) & 1u)) continue;
        const int tj = S.lt[j];
        if (!v_typed(tj)) continue;
        const float dx = xi - S.x[0][j], dy = yi - S.x[1][j], dz = zi - S.x[2][j];
        const float r2 = dx * dx + dy * dy + dz * dz;
        if (r2 >= V_CUTOFF * V_CUTOFF) continue;
        const float r = sqrtf(r2);
        float t5[5];
        const float de = pair_terms<true>(ti, tj, r, t5);
        if (SH::kFlex && (i >= nl || j >= nl)) {
          if (i < nl) { for (int k = 0; k < 5; ++k) acc[k] += (double)t5[k]; }
          else if (j >= nl && j > i) acc[NE - 1] += (double)t5[0] + (double)t5[1] + (double)t5[2] + (double)t5[3] + (double)t5[4];
        } else if (j > i) acc[5] += (double)t5[0] + (double)t5[1] + (double)t5[2] + (double)t5[3] + (double)t5[4];
        const float f = r > 0.f ? de / r : 0.f;
        gx += f * dx; gy += f * dy; gz += f * dz;
      }
    }
    gx = wsum(gx); gy = wsum(gy); gz = wsum(gz);
    if (lane == 0) { S.g[0][i] = gx; S.g[1][i] = gy; S.g[2][i] = gz; }
  }
  for (int k = 0; k < NE; ++k) acc[k] = wsumd(acc[k]);
  if (lane == 0)
    for (int k = 0; k < NE; ++k) S.red[w][k] = acc[k];
  __syncthreads();
  if (tid < NE) {
    double s = 0.0;
    for (int q = 0; q < V_WAVES; ++q) s += S.red[q][tid];
    S.e[tid] = s;
  }
  __syncthreads();
}

// Positions from the variables q = (t[3], rotation vector[3], torsions[nt]): S.y (torsions applied to x0) and S.x.
// The torsions act on all ns slots, the centroid and the rigid motion on the nl ligand atoms only.
template <class SH> __device__ void rebuild(SH& S, const float* q, int nl, int ns, int nt) {
  const int tid = threadIdx.x;
  for (int i = tid; i < ns; i += V_THREADS) { S.y[0][i] = S.x0[0][i]; S.y[1][i] = S.x0[1][i]; S.y[2][i] = S.x0[2][i]; }
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
      for (int i = tid; i < ns; i += V_THREADS)
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
    for (int i = tid; i < ns; i += V_THREADS) { S.x[0][i] = S.y[0][i]; S.x[1][i] = S.y[1][i]; S.x[2][i] = S.y[2][i]; }
    __syncthreads();
    return;
  }
  if constexpr (SH::kFlex)
    for (int i = nl + tid; i < ns; i += V_THREADS) { S.x[0][i] = S.y[0][i]; S.x[1][i] = S.y[1][i]; S.x[2][i] = S.y[2][i]; }
  for (int i = tid; i < nl; i += V_THREADS) {   // R (y - c) + c + t
    const float x = S.y[0][i] - S.c[0], y = S.y[1][i] - S.c[1], z = S.y[2][i] - S.c[2];
    S.x[0][i] = (S.R[0] * x + S.R[1] * y + S.R[2] * z) + S.c[0] + q[0];
    S.x[1][i] = (S.R[3] * x + S.R[4] * y + S.R[5] * z) + S.c[1] + q[1];
    S.x[2][i] = (S.R[6] * x + S.R[7] * y + S.R[8] * z) + S.c[2] + q[2];
  }
  __syncthreads();
}

// Gradient with respect to q from S.g = dE/dx (consumes S.g and S.y).  At q = 0 this is the generalised gradient.
// Receptor slots (nl .. ns - 1) do not follow the rigid motion: their dE/dx is the adjoint of their y already.
template <class SH> __device__ void param_grad(SH& S, const float* q, float* gq, int nl, int ns, int nt) {
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
    const bool in = tid < ns && ((S.tm[k][tid >> 5] >> (tid & 31)) & 1u);
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

// The pose's flexible receptor atoms, axis anchors, pairs and torsion masks into the slots behind the ligand's (see the head of
// the file).  Returns the number of slots, or -1 (uniformly) when a list of the graph is inconsistent or exceeds a capacity.
template <class SH> __device__ int flex_setup(const VinaArgs& A, SH& S, int g, int nl, int ntl, int na, int ne) {
  const int tid = threadIdx.x;
  const int a0 = A.b.atm_ptr[g];
  const int f0 = A.f_ptr[g], nf = A.f_ptr[g + 1] - f0;
  const int t0 = A.ft_ptr[g], ntf = A.ft_ptr[g + 1] - t0;
  for (int i = tid; i < V_FLEX_MAX_NA / 32; i += V_THREADS) S.fm[i] = 0u;
  __syncthreads();
  int bad = 0;
  for (int r = tid; r < nf; r += V_THREADS) {
    const int a = A.f_atom[f0 + r];
    if (a < 0 || a >= na) { bad = 1; continue; }
    S.fa[r] = a;
    bad |= (atomicOr(&S.fm[a >> 5], 1u << (a & 31)) >> (a & 31)) & 1u;   // listed twice
    for (int c = 0; c < 3; ++c) S.x0[c][nl + r] = S.x[c][nl + r] = S.xr[c][nl + r] = A.b.rec_pos[3 * (size_t)(a0 + a) + c];
    S.lt[nl + r] = A.in.rec_type[a0 + a];
    const int e0 = A.excl_ptr[f0 + r], e1 = A.excl_ptr[f0 + r + 1];
    bad |= e1 < e0 || e1 - e0 > V_FLEX_MAX_EXCL;
  }
  if (__syncthreads_or(bad)) return -1;
  // the two ends of every flexible torsion's axis: a flexible atom's slot, or -1 - (pocket atom) for an anchor still to place
  if (tid < 2 * ntf) {
    const int k = tid >> 1, a = A.ft_bc[2 * (size_t)(t0 + k) + (tid & 1)];
    int slot = -1 - a;
    if (a < 0 || a >= na) { bad = 1; slot = 0; }
    else if ((S.fm[a >> 5] >> (a & 31)) & 1u)
      for (int r = 0; r < nf; ++r)
        if (S.fa[r] == a) slot = nl + r;
    if (tid & 1) S.tu[ntl + k] = slot; else S.tv[ntl + k] = slot;   // pivot b = v, direction b -> c = u - v
  }
  __syncthreads();
  if (tid == 0) {
    int ns = nl + nf;
    for (int k = ntl; k < ntl + ntf; ++k)
      for (int end = 0; end < 2; ++end) {
        int& s = end ? S.tu[k] : S.tv[k];
        if (s >= 0) continue;
        if (ns < V_MAX_NL) {
          const int a = -1 - s;
          for (int c = 0; c < 3; ++c) S.x0[c][ns] = S.x[c][ns] = S.xr[c][ns] = A.b.rec_pos[3 * (size_t)(a0 + a) + c];
          S.lt[ns] = V_DUMMY;
          s = ns;
        } else s = 0;
        ++ns;
      }
    S.ncand = ns;   // (the candidate count is not in use yet: it carries the slot count to the other threads)
  }
  __syncthreads();
  const int ns = S.ncand;
  if (tid < ntf) bad |= S.tu[ntl + tid] == S.tv[ntl + tid];
  if (__syncthreads_or(bad || ns > V_MAX_NL)) return -1;
  // pairs: every flexible atom with every ligand atom and every other flexible atom ...
  const int nm = nl + nf;
  for (int idx = tid; idx < nf * nm; idx += V_THREADS) {
    const int s = nl + idx / nm, j = idx % nm;
    if (j == s) continue;
    atomicOr(&S.pm[s][j >> 5], 1u << (j & 31));
    atomicOr(&S.pm[j][s >> 5], 1u << (s & 31));
  }
  __syncthreads();
  // ... but the flexible atoms on its exclusion list
  for (int r = tid; r < nf; r += V_THREADS) {
    const int s = nl + r;
    for (int k = A.excl_ptr[f0 + r]; k < A.excl_ptr[f0 + r + 1]; ++k) {
      const int a = A.excl[k];
      if (a < 0 || a >= na + ne) { bad = 1; continue; }
      if (a >= na || !((S.fm[a >> 5] >> (a & 31)) & 1u)) continue;
      for (int h = 0; h < nf; ++h)
        if (S.fa[h] == a) {
          atomicAnd(&S.pm[s][(nl + h) >> 5], ~(1u << ((nl + h) & 31)));
          atomicAnd(&S.pm[nl + h][s >> 5], ~(1u << (s & 31)));
        }
    }
  }
  for (int k = 0; k < ntf; ++k) {
    const int m0 = A.turn_ptr[t0 + k], m1 = A.turn_ptr[t0 + k + 1];
    for (int m = m0 + tid; m < m1; m += V_THREADS) {
      const int r = A.turn[m];
      if (r < 0 || r >= nf) { bad = 1; continue; }
      atomicOr(&S.tm[ntl + k][(nl + r) >> 5], 1u << ((nl + r) & 31));
    }
  }
  if (__syncthreads_or(bad)) return -1;
  return ns;
}

// A graph the kernel will not touch: NaN terms, iters = -1.
template <int NT> __device__ __forceinline__ void refuse_pose(const VinaArgs& A, int g) {
  if (threadIdx.x < NT && A.terms) A.terms[NT * (size_t)g + threadIdx.x] = __int_as_float(0x7fc00000);
  if (threadIdx.x == 0 && A.iters) A.iters[g] = -1;
}

struct VinaDims { int l0, nl, k0, ntl, nt, ns, nf, n, na; };   // what vina_setup found of graph g

// Graph g into LDS: positions, types, pairs, torsion masks and axes (and the flexible slots).  Returns false (uniformly) for a graph
// the kernel will not touch.
template <class SH> __device__ __forceinline__ bool vina_setup(const VinaArgs& A, SH& S, int g, VinaDims& D) {
  const int tid = threadIdx.x;
  const VinaBatch& b = A.b;
  const int l0 = b.lig_ptr[g], nl = b.lig_ptr[g + 1] - l0;
  const int k0 = b.tor_ptr[g], ntl = b.tor_ptr[g + 1] - k0;
  int nt = ntl, ns = nl, nf = 0;
  if constexpr (SH::kFlex) { nt += A.ft_ptr[g + 1] - A.ft_ptr[g]; nf = A.f_ptr[g + 1] - A.f_ptr[g]; }
  const int n = 6 + nt;
  const int na = b.atm_ptr[g + 1] - b.atm_ptr[g], ne = A.in.ext_ptr ? A.in.ext_ptr[g + 1] - A.in.ext_ptr[g] : 0;
  bool refuse = nl <= 0 || nl > V_MAX_NL || ntl < 0 || nt > SH::kMaxVar - 6 || na < 0 || ne < 0 || na + ne > A.cap;
  if constexpr (SH::kFlex) refuse = refuse || nt < ntl || nf < 0 || nl + nf > V_MAX_NL || na > V_FLEX_MAX_NA;
  if (refuse) return false;   // the host-side maxima (max_nl, max_tor, max_na, max_ext, ...) understated this graph
  for (int i = tid; i < nl; i += V_THREADS) {
    for (int c = 0; c < 3; ++c) S.x0[c][i] = S.x[c][i] = S.xr[c][i] = b.lig_pos[3 * (size_t)(l0 + i) + c];
    S.lt[i] = A.in.lig_type[l0 + i];
  }
  for (int i = tid; i < V_MAX_NL * (V_MAX_NL / 32); i += V_THREADS) (&S.pm[0][0])[i] = 0u;
  for (int i = tid; i < nt * (V_MAX_NL / 32); i += V_THREADS) (&S.tm[0][0])[i] = 0u;
  __syncthreads();
  if constexpr (SH::kFlex) {
    ns = flex_setup(A, S, g, nl, ntl, na, ne);
    if (ns < 0) return false;   // an inconsistent flexible list, or more slots than the stated maxima allow
  }
  const int p0 = A.in.pair_ptr[g], np = A.in.pair_ptr[g + 1] - p0;
  for (int k = tid; k < np; k += V_THREADS) {
    const int i = A.in.pair_ij[2 * (size_t)(p0 + k)] - l0, j = A.in.pair_ij[2 * (size_t)(p0 + k) + 1] - l0;
    if (i < 0 || i >= nl || j < 0 || j >= nl) continue;
    atomicOr(&S.pm[i][j >> 5], 1u << (j & 31));   // integer bit sets: order-free
    atomicOr(&S.pm[j][i >> 5], 1u << (i & 31));
  }
  for (int k = 0; k < ntl; ++k) {
    const uint8_t* m = b.rot_mask + b.rot_mask_off[k0 + k];
    for (int i = tid; i < nl; i += V_THREADS)
      if (m[i]) atomicOr(&S.tm[k][i >> 5], 1u << (i & 31));
  }
  int bad = 0;
  if (tid < ntl) {
    const int e = b.tor_bond[k0 + tid];
    const int u = b.bond_src[e] - l0, v = b.bond_dst[e] - l0;
    bad = u < 0 || u >= nl || v < 0 || v >= nl || u == v;
    S.tu[tid] = bad ? 0 : u; S.tv[tid] = bad ? 0 : v;
  }
  if (__syncthreads_or(bad)) return false;   // a torsion bond outside the graph's atoms
  D = {l0, nl, k0, ntl, nt, ns, nf, n, na};
  return true;
}

// BFGS from S.pn (S.p = 0, S.H = I) over the variables of `rebuild`, whose base S.x0 is: at most max_iters accepted steps.  Leaves
// the final positions in S.x and their terms in S.e; returns the accepted steps.  rec0: E_rec of the first evaluation (flexible).
template <class SH> __device__ __forceinline__ int vina_bfgs(const VinaArgs& A, SH& S, int g, const VinaDims& D, int max_iters, double& rec0) {
  const int tid = threadIdx.x;
  const int nl = D.nl, ns = D.ns, nt = D.nt, n = D.n;
  // One evaluation per pass (a single call site of rebuild / evaluate / param_grad each keeps the scalar registers in
  // budget): phase 0 = the start q = 0, 1 = a line-search trial at pn = p + alpha d, 2 = back to p after a stalled search.
  int phase = 0, it = 0, ls = 0;
  bool identity = true;
  double f = 0.0;
  float alpha = 0.f, slope = 0.f;
  for (;;) {
    rebuild(S, S.pn, nl, ns, nt);
    evaluate(A, S, g, nl, ns);
    double fn = S.e[0] + S.e[1] + S.e[2] + S.e[3] + S.e[4] + S.e[5];
    if constexpr (SH::kFlex) {
      fn += S.e[6];
      if (phase == 0) rec0 = S.e[6];
    }
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
      param_grad(S, S.pn, S.gn, nl, ns, nt);
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
    if (gmax < A.grad_tol || it >= max_iters) {
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
  return it;
}

template <class SH> __device__ __forceinline__ void vina_pose(const VinaArgs& A, SH& S) {
  constexpr int NT = SH::kFlex ? 10 : 8;   // terms per pose
  const int g = blockIdx.x, tid = threadIdx.x;
  const VinaBatch& b = A.b;
  VinaDims D;
  if (!vina_setup(A, S, g, D)) {   // NaN results, nothing touched
    refuse_pose<NT>(A, g);
    return;
  }
  const int l0 = D.l0, nl = D.nl, k0 = D.k0, ntl = D.ntl, nt = D.nt, nf = D.nf, n = D.n, na = D.na;
  for (int k = tid; k < SH::kMaxVar; k += V_THREADS) {
    S.p[k] = 0.f;
    S.pn[k] = k < 6 ? (A.q_rigid ? A.q_rigid[6 * (size_t)g + k] : 0.f) : (k < 6 + ntl && A.q_tor ? A.q_tor[k0 + k - 6] : 0.f);
    if constexpr (SH::kFlex)
      if (k >= 6 + ntl && k < n && A.q_flex) S.pn[k] = A.q_flex[A.ft_ptr[g] + k - 6 - ntl];
  }
  for (int i = tid; i < n * n; i += V_THREADS) S.H[i] = (i / n == i % n) ? 1.f : 0.f;
  if (tid == 0) S.flag = 1;   // collect the candidates at the first evaluation
  __syncthreads();
  double rec0 = 0.0;
  const int it = vina_bfgs(A, S, g, D, A.max_iters, rec0);
  if (tid == 0) {
    if (A.terms) {
      float* t = A.terms + NT * (size_t)g;
      double inter = 0.0;
      for (int k = 0; k < 5; ++k) { t[k] = (float)S.e[k]; inter += S.e[k]; }
      t[5] = (float)S.e[5];
      t[6] = (float)(inter + S.e[5]);
      t[7] = (float)(inter / (1.0 + (double)W_NROT * ntl));
      if constexpr (SH::kFlex) { t[6] = (float)(inter + S.e[5] + S.e[6]); t[8] = (float)S.e[6]; t[9] = (float)rec0; }
    }
    if (A.iters) A.iters[g] = it;
  }
  if (!A.minimize) {
    if (A.grad_rigid && tid < 6) A.grad_rigid[6 * (size_t)g + tid] = S.gp[tid];
    if (A.grad_tor && tid < ntl) A.grad_tor[k0 + tid] = S.gp[6 + tid];
    if constexpr (SH::kFlex)
      if (A.grad_flex && tid < nt - ntl) A.grad_flex[A.ft_ptr[g] + tid] = S.gp[6 + ntl + tid];
  }
  if (A.pos_out)
    for (int i = tid; i < nl; i += V_THREADS)
      for (int c = 0; c < 3; ++c) A.pos_out[3 * (size_t)(l0 + i) + c] = S.x[c][i];
  if constexpr (SH::kFlex) {
    if (A.q_flex_out && tid < nt - ntl) A.q_flex_out[A.ft_ptr[g] + tid] = S.p[6 + ntl + tid];
    if (A.rec_out) {   // the pocket atoms: fixed ones copied, flexible ones from their slots
      const size_t a0 = (size_t)b.atm_ptr[g];
      for (int c = tid; c < na; c += V_THREADS)
        if (!((S.fm[c >> 5] >> (c & 31)) & 1u))
          for (int k = 0; k < 3; ++k) A.rec_out[3 * (a0 + c) + k] = b.rec_pos[3 * (a0 + c) + k];
      for (int r = tid; r < nf; r += V_THREADS)
        for (int k = 0; k < 3; ++k) A.rec_out[3 * (a0 + S.fa[r]) + k] = S.x[k][nl + r];
    }
  }
}

template <int MT> __global__ __launch_bounds__(V_THREADS) void k_vina(VinaArgs A) {
  using SH = VinaShared<MT>;
  if constexpr (SH::kFlex) {   // 105 KB: dynamic LDS (hipFuncAttributeMaxDynamicSharedMemorySize)
    extern __shared__ __align__(16) unsigned char v_lds[];
    vina_pose(A, *reinterpret_cast<SH*>(v_lds));
  } else {
    __shared__ SH S;
    vina_pose(A, S);
  }
}

// ------------------------------------------------------------------------------------------------ Monte-Carlo search
// Vina's iterated local search around the minimiser above (include/dbfr.h: dbfr_vina_search; docs/vina.md, "Monte-Carlo search").
// One workgroup per (pose, chain), block = chain * G + pose.  The chain's current pose is the base S.x0 of `rebuild`, so a mutation
// is a q with one entity set; the best pose lives in xb.  Random numbers are Philox4x32-10 blocks addressed by (seed; stream, chain,
// slot): nothing is carried from draw to draw, and nothing of a chain depends on another workgroup.
struct Philox4 { uint32_t w[4]; };

__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return {{c0, c1, c2, c3}};
}

__host__ __device__ inline float philox_u(uint32_t w) { return (float)(w >> 8) * (1.f / 16777216.f); }   // [0, 1)

struct VinaRng {          // one (pose, chain)
  uint32_t k0, k1, s0, s1, chain;
  __host__ __device__ Philox4 slot(uint32_t s) const { return philox4x32_10(s0, s1, chain, s, k0, k1); }
};

__host__ __device__ inline VinaRng vina_rng(uint64_t seed, int64_t stream, int chain) {
  return {(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)(uint64_t)stream, (uint32_t)((uint64_t)stream >> 32), (uint32_t)chain};
}

#define V_TWO_PI 6.28318530717958647692f
#define V_PI 3.14159265358979323846f

// The mutation of Monte-Carlo step `step` (1-based): q[0 .. 6 + n_tor) is zero but for the chosen entity; returns the entity.
__host__ __device__ inline int vina_mutation(const VinaRng& rng, int step, int n_tor, float amplitude, float r_g, float* q) {
  const Philox4 r = rng.slot(2u * (uint32_t)step);
  const int e = (int)(((uint64_t)r.w[0] * (uint64_t)(2 + n_tor)) >> 32);
  const float u1 = philox_u(r.w[1]), u2 = philox_u(r.w[2]), u3 = philox_u(r.w[3]);
  for (int k = 0; k < 6 + n_tor; ++k) q[k] = 0.f;
  if (e >= 2) { q[6 + e - 2] = V_TWO_PI * u1 - V_PI; return e; }
  const float z = 2.f * u1 - 1.f, phi = V_TWO_PI * u2, rho = cbrtf(u3);
  const float s = sqrtf(fmaxf(1.f - z * z, 0.f));
  const float a = e == 0 ? amplitude : amplitude / r_g;
  q[3 * e + 0] = a * (rho * (s * cosf(phi)));
  q[3 * e + 1] = a * (rho * (s * sinf(phi)));
  q[3 * e + 2] = a * (rho * z);
  return e;
}

// A random placement's variables but the translation (which needs the centroid after the torsions: k_vina_search): Shoemake's
// uniform unit quaternion (x, y, z, w) from three uniforms as the rotation vector 2 atan2(|v|, w) v / |v|, and uniform torsions.
__host__ __device__ inline void vina_random_start(const VinaRng& rng, int n_tor, float* q) {
  const Philox4 r = rng.slot(1u);
  const float u1 = philox_u(r.w[1]), u2 = philox_u(r.w[2]), u3 = philox_u(r.w[3]);
  const float a = sqrtf(1.f - u1), b = sqrtf(u1);
  const float x = a * sinf(V_TWO_PI * u2), y = a * cosf(V_TWO_PI * u2), z = b * sinf(V_TWO_PI * u3), w = b * cosf(V_TWO_PI * u3);
  const float nv = sqrtf(x * x + y * y + z * z);
  const float f = nv > 0.f ? 2.f * atan2f(nv, w) / nv : 0.f;
  q[0] = q[1] = q[2] = 0.f;
  q[3] = f * x; q[4] = f * y; q[5] = f * z;
  for (int k = 0; k < n_tor; ++k) q[6 + k] = V_TWO_PI * philox_u(rng.slot(0x80000000u + (uint32_t)k).w[0]) - V_PI;
}

struct VinaSearchArgs {
  int G, chains, n_steps, step_iters, random_start;
  float temperature, amplitude, autobox_add;
  uint64_t seed;
  const int64_t* stream;   // [G]
  float *best_pos, *cur_pos;   // [chains, NL, 3]
  int* accepted;           // [chains, G]
  float* log;              // [chains, G, n_steps, 8] or null
  size_t NL;
  // flexible instantiation only
  float *best_rec, *cur_rec;   // [chains, NA, 3] (cur_rec or null)
  float* q_flex_out;       // [chains, NFT]
  size_t NA, NFT;
};

// The search state behind the minimiser's struct.  Flexible: the best pose and the base cover all slots, and two accumulators carry
// the total flexible torsion angles of the current (qc) and the best (qb) pose through the re-basing.
template <bool F> struct VinaSearchFlexShared {};
template <> struct VinaSearchFlexShared<true> {
  float qc[V_FLEX_MAX_TOR], qb[V_FLEX_MAX_TOR];
};
template <int MT> struct VinaSearchShared : VinaShared<MT>, VinaSearchFlexShared<(MT > V_MAX_TOR)> {
  float xb[3][V_MAX_NL];   // the chain's best pose
  double eb[VinaShared<MT>::kFlex ? 8 : 6];   // and its terms
  float lo[3], hi[3];      // the box
  float rg;                // radius of gyration of the input pose
  int ent;                 // the step's entity
};
static_assert(sizeof(VinaSearchShared<V_MAX_TOR>) <= (160 * 1024) / 3, "three search workgroups per CU");
static_assert(sizeof(VinaSearchShared<V_FLEX_MAX_TOR>) <= 160 * 1024 - 64, "the flexible search must fit the gfx950 workgroup LDS limit");

template <bool F> __device__ __forceinline__ float v_objective(const double* e) {
  double inter = 0.0;
  for (int k = 0; k < 5; ++k) inter += e[k];
  if constexpr (F) return (float)(inter + e[5] + e[6]);
  return (float)(inter + e[5]);
}

__device__ __forceinline__ float v_wrap_pi(float a) {   // into [-pi, pi); a value inside keeps its bits
  while (a >= V_PI) a -= V_TWO_PI;
  while (a < -V_PI) a += V_TWO_PI;
  return a;
}

// The pocket atoms of slots `x` (S.x0 or S.xb) into out [NA, 3] of this chain: fixed ones copied, flexible ones from their slots.
template <class SH> __device__ __forceinline__ void search_rec_out(const VinaArgs& A, SH& S, const float (*x)[V_MAX_NL], float* out,
                                                                 int g, const VinaDims& D) {
  const size_t a0 = (size_t)A.b.atm_ptr[g];
  for (int c = threadIdx.x; c < D.na; c += V_THREADS)
    if (!((S.fm[c >> 5] >> (c & 31)) & 1u))
      for (int k = 0; k < 3; ++k) out[3 * (a0 + c) + k] = A.b.rec_pos[3 * (a0 + c) + k];
  for (int r = threadIdx.x; r < D.nf; r += V_THREADS)
    for (int k = 0; k < 3; ++k) out[3 * (a0 + S.fa[r]) + k] = x[k][D.nl + r];
}

template <class SH> __device__ __forceinline__ void vina_search_chain(VinaArgs A, const VinaSearchArgs& Q, SH& S) {
  constexpr bool F = SH::kFlex;
  constexpr int NT = F ? 10 : 8, NE = F ? 7 : 6;
  const int tid = threadIdx.x;
  const int g = blockIdx.x % Q.G, chain = blockIdx.x / Q.G;
  const size_t blk = blockIdx.x;
  // this chain's slices of the workspace and of the per-pose outputs: the device functions index them by g
  A.cand += (size_t)chain * Q.G * A.cap;
  A.terms += NT * (size_t)chain * Q.G;
  A.iters += (size_t)chain * Q.G;
  VinaDims D;
  if (!vina_setup(A, S, g, D)) {   // NaN terms, iters = -1, nothing touched
    refuse_pose<NT>(A, g);
    if (tid == 0) Q.accepted[blk] = 0;
    return;
  }
  const int l0 = D.l0, nl = D.nl, nt = D.nt, n = D.n;
  const int nb = F ? D.ns : nl;        // the slots of the base and of the best pose
  const int ntl = D.ntl, nft = nt - ntl;
  const VinaRng rng = vina_rng(Q.seed, Q.stream[g], chain);
  // the box and the radius of gyration of the input pose (the ligand's atoms)
  if (tid < 3) {
    float lo = S.x0[tid][0], hi = lo, s = 0.f;
    for (int i = 0; i < nl; ++i) { const float v = S.x0[tid][i]; lo = fminf(lo, v); hi = fmaxf(hi, v); s += v; }
    S.lo[tid] = lo - Q.autobox_add; S.hi[tid] = hi + Q.autobox_add; S.c[tid] = s / (float)nl;
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int i = 0; i < nl; ++i) {
      const float dx = S.x0[0][i] - S.c[0], dy = S.x0[1][i] - S.c[1], dz = S.x0[2][i] - S.c[2];
      s += dx * dx + dy * dy + dz * dz;
    }
    S.rg = fmaxf(sqrtf(s / (float)nl), 1e-3f);
    S.flag = 1;   // collect the candidates at the first evaluation
  }
  __syncthreads();
  const int step_iters = Q.step_iters < 0 ? (25 + nl + D.nf) / 3 : Q.step_iters;
  // stage -1: a random placement (evaluated, not minimised); 0: the start minimisation; 1 .. n_steps: the Monte-Carlo steps;
  // n_steps + 1: the final refinement of a best that came from a step.  (One call site of vina_bfgs, as in vina_pose.)
  int stage = (Q.random_start && chain >= 1) ? -1 : 0;
  int total = 0, nacc = 0;
  bool best_from_step = false;
  float e_cur = 0.f, e_best = 0.f;
  double rec_start = 0.0;
  for (;;) {
    for (int k = tid; k < SH::kMaxVar; k += V_THREADS) { S.p[k] = 0.f; S.pn[k] = 0.f; }
    for (int i = tid; i < n * n; i += V_THREADS) S.H[i] = (i / n == i % n) ? 1.f : 0.f;
    __syncthreads();
    if (tid == 0) {
      if (stage == -1) vina_random_start(rng, ntl, S.pn);   // the ligand only: flexible torsions start as sampled
      else if (stage >= 1 && stage <= Q.n_steps) S.ent = vina_mutation(rng, stage, nt, Q.amplitude, S.rg, S.pn);
    }
    __syncthreads();
    double rec0 = 0.0;
    const int it = vina_bfgs(A, S, g, D, stage == -1 ? 0 : (stage >= 1 && stage <= Q.n_steps) ? step_iters : A.max_iters, rec0);
    total += it;
    __syncthreads();
    const float e_c = v_objective<F>(S.e);
    bool in_box = true;
    if (stage == -1) {
      // the rotation was about the centroid S.c of the turned ligand, which is therefore still the centroid: move it to its draw
      const Philox4 r = rng.slot(0u);
      float sh[3];
      for (int c = 0; c < 3; ++c) sh[c] = (S.lo[c] + philox_u(r.w[1 + c]) * (S.hi[c] - S.lo[c])) - S.c[c];
      __syncthreads();
      for (int i = tid; i < nl; i += V_THREADS)
        for (int c = 0; c < 3; ++c) S.x0[c][i] = S.x[c][i] + sh[c];
    } else if (stage == 0) {
      for (int i = tid; i < nb; i += V_THREADS)
        for (int c = 0; c < 3; ++c) S.x0[c][i] = S.xb[c][i] = S.x[c][i];
      if (tid < NE) S.eb[tid] = S.e[tid];
      if constexpr (F) {
        if (tid < nft) S.qc[tid] = S.qb[tid] = v_wrap_pi(S.p[6 + ntl + tid]);
        rec_start = rec0;
      }
      e_cur = e_best = e_c;
    } else {
      int out = 0;
      for (int i = tid; i < nl; i += V_THREADS)
        for (int c = 0; c < 3; ++c) out |= !(S.x[c][i] >= S.lo[c] && S.x[c][i] <= S.hi[c]);
      in_box = !__syncthreads_or(out);
    }
    if (stage >= 1 && stage <= Q.n_steps) {
      const float u = philox_u(rng.slot(2u * (uint32_t)stage + 1u).w[0]);
      // (expf: its error on a threshold below 1 is under 1e-7, and the double-precision exp costs 21 VGPRs and a wave per SIMD)
      const bool accept = in_box && (e_c < e_cur || u < expf((e_cur - e_c) / Q.temperature));
      if (accept) {
        const bool better = e_c < e_best;
        for (int i = tid; i < nb; i += V_THREADS)
          for (int c = 0; c < 3; ++c) {
            S.x0[c][i] = S.x[c][i];
            if (better) S.xb[c][i] = S.x[c][i];
          }
        if constexpr (F)
          if (tid < nft) {
            const float a = v_wrap_pi(S.qc[tid] + S.p[6 + ntl + tid]);
            S.qc[tid] = a;
            if (better) S.qb[tid] = a;
          }
        if (better) {
          if (tid < NE) S.eb[tid] = S.e[tid];
          e_best = e_c;
          best_from_step = true;
        }
        e_cur = e_c;
        ++nacc;
      }
      if (Q.log && tid == 0) {
        float* L = Q.log + 8 * ((size_t)blk * Q.n_steps + (stage - 1));
        L[0] = (float)S.ent; L[1] = e_c; L[2] = in_box ? 1.f : 0.f; L[3] = u; L[4] = accept ? 1.f : 0.f;
        L[5] = e_cur; L[6] = e_best; L[7] = (float)it;
      }
    } else if (stage > Q.n_steps) {   // the refined best, kept if it is not higher and has not left the box
      if (in_box && e_c <= e_best) {
        for (int i = tid; i < nb; i += V_THREADS)
          for (int c = 0; c < 3; ++c) S.xb[c][i] = S.x[c][i];
        if (tid < NE) S.eb[tid] = S.e[tid];
        if constexpr (F)
          if (tid < nft) S.qb[tid] = v_wrap_pi(S.qb[tid] + S.p[6 + ntl + tid]);
      }
    }
    __syncthreads();
    if (stage > Q.n_steps) break;
    if (stage == Q.n_steps) {   // the chain's current pose; then the best becomes the base of the refinement
      if (Q.cur_pos)
        for (int i = tid; i < nl; i += V_THREADS)
          for (int c = 0; c < 3; ++c) Q.cur_pos[3 * (Q.NL * chain + l0 + i) + c] = S.x0[c][i];
      if constexpr (F)
        if (Q.cur_rec) search_rec_out(A, S, S.x0, Q.cur_rec + 3 * Q.NA * chain, g, D);
      if (!best_from_step) break;
      __syncthreads();
      for (int i = tid; i < nb; i += V_THREADS)
        for (int c = 0; c < 3; ++c) S.x0[c][i] = S.xb[c][i];
    }
    ++stage;
  }
  __syncthreads();
  if (tid == 0) {
    float* t = A.terms + NT * (size_t)g;
    double inter = 0.0;
    for (int k = 0; k < 5; ++k) { t[k] = (float)S.eb[k]; inter += S.eb[k]; }
    t[5] = (float)S.eb[5];
    t[6] = (float)(inter + S.eb[5]);
    t[7] = (float)(inter / (1.0 + (double)W_NROT * D.ntl));
    if constexpr (F) { t[6] = (float)(inter + S.eb[5] + S.eb[6]); t[8] = (float)S.eb[6]; t[9] = (float)rec_start; }
    A.iters[g] = total;
    Q.accepted[blk] = nacc;
  }
  for (int i = tid; i < nl; i += V_THREADS)
    for (int c = 0; c < 3; ++c) Q.best_pos[3 * (Q.NL * chain + l0 + i) + c] = S.xb[c][i];
  if constexpr (F) {
    search_rec_out(A, S, S.xb, Q.best_rec + 3 * Q.NA * chain, g, D);
    if (tid < nft) Q.q_flex_out[Q.NFT * chain + A.ft_ptr[g] + tid] = S.qb[tid];
  }
}

template <int MT> __global__ __launch_bounds__(V_THREADS) void k_vina_search(VinaArgs A, VinaSearchArgs Q) {
  using SH = VinaSearchShared<MT>;
  if constexpr (SH::kFlex) {   // dynamic LDS, as k_vina<flex>
    extern __shared__ __align__(16) unsigned char v_lds[];
    vina_search_chain(A, Q, *reinterpret_cast<SH*>(v_lds));
  } else {
    __shared__ SH S;
    vina_search_chain(A, Q, S);
  }
}

extern "C" int dbfr_test_philox4x32(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
  if (!ctr || !key || !out) { dbfr_set_error("dbfr_test_philox4x32: null argument"); return DBFR_ERR_ARG; }
  const Philox4 r = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
  for (int k = 0; k < 4; ++k) out[k] = r.w[k];
  return DBFR_OK;
}

extern "C" int dbfr_test_vina_mutation(uint64_t seed, int64_t stream, int32_t chain, int32_t step, int32_t n_tor, float amplitude, float r_g,
                                       int32_t* entity, float* q) {
  if (!entity || !q || n_tor < 0 || step < 1 || chain < 0 || !(r_g > 0.f)) {
    dbfr_set_error("dbfr_test_vina_mutation: entity and q [6 + n_tor], n_tor >= 0, step >= 1, chain >= 0 and r_g > 0 required");
    return DBFR_ERR_ARG;
  }
  *entity = vina_mutation(vina_rng(seed, stream, chain), step, n_tor, amplitude, r_g, q);
  return DBFR_OK;
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

// ---- flexible side chains: the checks of dbfr_vina_flex_in
static int vf_err(const std::string& s) { dbfr_set_error("dbfr_vina_flex: " + s); return DBFR_ERR_ARG; }

// every list of the host copies: CSR shapes, index ranges, the per-graph counts against the stated maxima
static int vina_flex_validate(const dbfr_vina_flex_in& in, const dbfr_vina_flex_in& h, int G, int max_na, int max_ext) {
  if (!h.flex_ptr || !h.ftor_ptr || (in.n_flex > 0 && (!h.flex_atom || !h.excl_ptr)) || (in.n_ftor > 0 && (!h.ftor_bc || !h.turn_ptr)))
    return vf_err("host: a host copy of an index array is missing");
  if (h.flex_ptr[0] != 0 || h.ftor_ptr[0] != 0 || h.flex_ptr[G] != in.n_flex || h.ftor_ptr[G] != in.n_ftor)
    return vf_err("flex_ptr / ftor_ptr must run from 0 to n_flex / n_ftor");
  if (in.n_flex > 0 && h.excl_ptr[0] != 0) return vf_err("excl_ptr must start at 0");
  if (in.n_ftor > 0 && h.turn_ptr[0] != 0) return vf_err("turn_ptr must start at 0");
  if ((in.n_flex > 0 && h.excl_ptr[in.n_flex] > 0 && !h.excl) || (in.n_ftor > 0 && h.turn_ptr[in.n_ftor] > 0 && !h.turn))
    return vf_err("host: a host copy of an index array is missing");
  for (int g = 0; g < G; ++g) {
    const int f0 = h.flex_ptr[g], nf = h.flex_ptr[g + 1] - f0, t0 = h.ftor_ptr[g], nt = h.ftor_ptr[g + 1] - t0;
    const std::string where = "graph " + std::to_string(g) + ": ";
    if (nf < 0 || nt < 0) return vf_err(where + "flex_ptr / ftor_ptr must not decrease");
    if (nf > in.max_flex) return vf_err(where + std::to_string(nf) + " flexible atoms, max_flex states " + std::to_string(in.max_flex));
    if (nt > in.max_ftor) return vf_err(where + std::to_string(nt) + " flexible torsions, max_ftor states " + std::to_string(in.max_ftor));
    for (int r = 0; r < nf; ++r) {
      const int a = h.flex_atom[f0 + r];
      if (a < 0 || a >= max_na) return vf_err(where + "flexible atom " + std::to_string(a) + " is out of range (pocket atoms 0.." + std::to_string(max_na - 1) + ")");
      if (r && a <= h.flex_atom[f0 + r - 1]) return vf_err(where + "flexible atoms must ascend");
      const int e0 = h.excl_ptr[f0 + r], e1 = h.excl_ptr[f0 + r + 1];
      if (e1 < e0) return vf_err(where + "excl_ptr must not decrease");
      if (e1 - e0 > in.max_excl)
        return vf_err(where + "exclusion list of " + std::to_string(e1 - e0) + " atoms, max_excl states " + std::to_string(in.max_excl) + " (at most 32)");
      for (int k = e0; k < e1; ++k)
        if (h.excl[k] < 0 || h.excl[k] >= max_na + max_ext)
          return vf_err(where + "excluded receptor atom " + std::to_string(h.excl[k]) + " is out of range");
    }
    int anchors = 0;
    for (int k = 0; k < nt; ++k) {
      const int bc[2] = {h.ftor_bc[2 * (size_t)(t0 + k)], h.ftor_bc[2 * (size_t)(t0 + k) + 1]};
      if (bc[0] == bc[1]) return vf_err(where + "a flexible torsion's axis needs two different atoms");
      for (int a : bc) {
        if (a < 0 || a >= max_na) return vf_err(where + "torsion axis atom " + std::to_string(a) + " is out of range (pocket atoms 0.." + std::to_string(max_na - 1) + ")");
        anchors += !std::binary_search(h.flex_atom + f0, h.flex_atom + f0 + nf, a);
      }
      const int m0 = h.turn_ptr[t0 + k], m1 = h.turn_ptr[t0 + k + 1];
      if (m1 < m0) return vf_err(where + "turn_ptr must not decrease");
      for (int m = m0; m < m1; ++m)
        if (h.turn[m] < 0 || h.turn[m] >= nf)
          return vf_err(where + "turned atom " + std::to_string(h.turn[m]) + " is out of range (the graph's " + std::to_string(nf) + " flexible atoms)");
    }
    if (anchors > in.max_anchor)
      return vf_err(where + std::to_string(anchors) + " axis anchors, max_anchor states " + std::to_string(in.max_anchor));
  }
  return DBFR_OK;
}

static int vina_flex_check(const dbfr_vina_flex_in* in, size_t* cap_per_pose) {
  if (!in || !in->base) { dbfr_set_error("dbfr_vina_flex: null argument"); return DBFR_ERR_ARG; }
  const int rc = vina_check(in->base, cap_per_pose);
  if (rc) return rc;
  const dbfr_batch* b = in->base->batch;
  if (in->n_flex < 0 || in->n_ftor < 0 || in->max_flex < 0 || in->max_ftor < 0 || in->max_anchor < 0 || in->max_excl < 0)
    return vf_err("counts and maxima must be >= 0");
  if (b->max_nl + in->max_flex + in->max_anchor > V_MAX_NL)
    return vf_err(std::to_string(b->max_nl) + " ligand atoms + " + std::to_string(in->max_flex) + " flexible atoms + " +
                  std::to_string(in->max_anchor) + " axis anchors: at most 256 together");
  if (6 + in->base->max_tor + in->max_ftor > 6 + V_FLEX_MAX_TOR)
    return vf_err(std::to_string(6 + in->base->max_tor + in->max_ftor) + " variables (6 + " + std::to_string(in->base->max_tor) +
                  " ligand torsions + " + std::to_string(in->max_ftor) + " flexible torsions): at most 128");
  if (in->max_excl > V_FLEX_MAX_EXCL) return vf_err("exclusion lists of " + std::to_string(in->max_excl) + " atoms: at most 32");
  if (!in->flex_ptr || !in->ftor_ptr || (in->n_flex > 0 && (!in->flex_atom || !in->excl_ptr)) ||
      (in->n_ftor > 0 && (!in->ftor_bc || !in->turn_ptr)))
    return vf_err("null device pointer in the input");
  if (in->host) return vina_flex_validate(*in, *static_cast<const dbfr_vina_flex_in*>(in->host), b->G, b->max_na,
                                          in->base->ext_ptr ? in->base->max_ext : 0);
  return DBFR_OK;
}

struct VinaFlexOut { const float* q_flex; float *rec_out, *q_flex_out, *grad_flex; };

// The kernel arguments every launch shares: the batch, the candidate workspace and the minimiser's options.
static int vina_args(const dbfr_vina_in* in, const dbfr_vina_opts* opts, size_t cap, void* ws, VinaArgs& A) {
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
  return DBFR_OK;
}

static int vina_launch(const dbfr_vina_in* in, int minimize, const dbfr_vina_opts* opts, const float* q_rigid, const float* q_tor,
                       float* pos_out, float* terms, float* grad_rigid, float* grad_tor, int32_t* iters, void* ws, size_t ws_bytes,
                       void* stream, const dbfr_vina_flex_in* flex = nullptr, const VinaFlexOut* fo = nullptr) {
  size_t cap;
  int rc = flex ? vina_flex_check(flex, &cap) : vina_check(in, &cap);
  if (rc) return rc;
  const size_t need = (size_t)in->batch->G * cap * sizeof(float4);
  if (!ws || ws_bytes < need) {
    dbfr_set_error("dbfr_vina: workspace of " + std::to_string(ws_bytes) + " bytes, this batch needs " + std::to_string(need) +
                   " (dbfr_vina_workspace_bytes)");
    return DBFR_ERR_ARG;
  }
  VinaArgs A;
  rc = vina_args(in, opts, cap, ws, A);
  if (rc) return rc;
  A.minimize = minimize;
  A.q_rigid = q_rigid; A.q_tor = in->batch->NTOR > 0 ? q_tor : nullptr;
  A.pos_out = pos_out; A.terms = terms; A.grad_rigid = grad_rigid; A.grad_tor = grad_tor; A.iters = iters;
  if (flex) {
    A.f_ptr = flex->flex_ptr; A.f_atom = flex->flex_atom; A.ft_ptr = flex->ftor_ptr; A.ft_bc = flex->ftor_bc;
    A.turn_ptr = flex->turn_ptr; A.turn = flex->turn; A.excl_ptr = flex->excl_ptr; A.excl = flex->excl;
    A.q_flex = flex->n_ftor > 0 ? fo->q_flex : nullptr;
    A.rec_out = fo->rec_out; A.q_flex_out = fo->q_flex_out; A.grad_flex = fo->grad_flex;
    // (the LDS attribute is set on every launch: it is per device, and a process may drive several)
    const size_t lds = sizeof(VinaShared<V_FLEX_MAX_TOR>);
    if (dbfr_launch_check(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_vina<V_FLEX_MAX_TOR>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                          "k_vina<flex>: hipFuncSetAttribute(MaxDynamicSharedMemorySize)"))
      return dbfr_take_launch_error();
    hipLaunchKernelGGL(k_vina<V_FLEX_MAX_TOR>, dim3(in->batch->G), dim3(V_THREADS), lds, (hipStream_t)stream, A);
  } else {
    hipLaunchKernelGGL(k_vina<V_MAX_TOR>, dim3(in->batch->G), dim3(V_THREADS), 0, (hipStream_t)stream, A);
  }
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

static int vina_search_check(const dbfr_vina_in* in, int64_t chains, size_t* cap, const dbfr_vina_flex_in* flex = nullptr) {
  const int rc = flex ? vina_flex_check(flex, cap) : vina_check(in, cap);
  if (rc) return rc;
  if (flex) in = flex->base;
  if (chains < 1) { dbfr_set_error("dbfr_vina_search: chains >= 1 required"); return DBFR_ERR_ARG; }
  if ((int64_t)in->batch->G * chains > 0x7fffffff) {
    dbfr_set_error("dbfr_vina_search: " + std::to_string(in->batch->G) + " poses x " + std::to_string(chains) + " chains exceed the grid of 2^31 - 1 workgroups");
    return DBFR_ERR_ARG;
  }
  return DBFR_OK;
}

extern "C" int dbfr_vina_search_workspace_bytes(const dbfr_vina_in* in, int32_t chains, size_t* bytes) {
  size_t cap;
  const int rc = vina_search_check(in, chains, &cap);
  if (rc) return rc;
  if (!bytes) { dbfr_set_error("dbfr_vina_search_workspace_bytes: null argument"); return DBFR_ERR_ARG; }
  *bytes = (size_t)chains * in->batch->G * cap * sizeof(float4);
  return DBFR_OK;
}

struct VinaSearchFlexOut { float *best_rec, *q_flex_out, *cur_rec; };

// dbfr_vina_search and dbfr_vina_flex_search: the checks in one order, then the rigid or the flexible instantiation.
static int vina_search_launch(const char* name, const dbfr_vina_in* in, const dbfr_vina_opts* opts, const dbfr_vina_search_opts* search_opts,
                              const int64_t* stream, float* best_pos, float* cur_pos, float* terms, int32_t* iters, int32_t* accepted,
                              float* log, void* workspace, size_t workspace_bytes, void* hip_stream,
                              const dbfr_vina_flex_in* flex = nullptr, const VinaSearchFlexOut* fo = nullptr) {
  const std::string who = name;
  dbfr_vina_search_opts so = {8, 64, -1, 1.2f, 2.f, 4.f, 0, 0};
  if (search_opts) so = *search_opts;
  size_t cap;
  int rc = vina_search_check(in, so.chains, &cap, flex);
  if (rc) return rc;
  if (so.n_steps < 0 || !(so.temperature > 0.f) || !(so.amplitude >= 0.f) || !(so.autobox_add >= 0.f)) {
    dbfr_set_error(who + ": n_steps >= 0, temperature > 0, amplitude >= 0 and autobox_add >= 0 required");
    return DBFR_ERR_ARG;
  }
  if (!stream || !best_pos || !terms || !iters || !accepted) {
    dbfr_set_error(who + ": stream, best_pos, terms, iters and accepted are required");
    return DBFR_ERR_ARG;
  }
  if (flex && (!fo->best_rec || (flex->n_ftor > 0 && !fo->q_flex_out))) {
    dbfr_set_error(who + ": best_rec and q_flex_out are required");
    return DBFR_ERR_ARG;
  }
  const dbfr_batch* B = in->batch;
  const size_t need = (size_t)so.chains * B->G * cap * sizeof(float4);
  if (!workspace || workspace_bytes < need) {
    dbfr_set_error(who + ": workspace of " + std::to_string(workspace_bytes) + " bytes, this batch needs " + std::to_string(need) +
                   " (" + who + "_workspace_bytes)");
    return DBFR_ERR_ARG;
  }
  VinaArgs A;
  rc = vina_args(in, opts, cap, workspace, A);
  if (rc) return rc;
  A.minimize = 1;
  A.terms = terms; A.iters = iters;
  VinaSearchArgs Q = {B->G, so.chains, so.n_steps, so.step_iters, so.random_start, so.temperature, so.amplitude, so.autobox_add,
                      so.seed, stream, best_pos, cur_pos, accepted, log, (size_t)B->NL, nullptr, nullptr, nullptr, 0, 0};
  const dim3 grid((unsigned)(B->G * so.chains));
  if (flex) {
    A.f_ptr = flex->flex_ptr; A.f_atom = flex->flex_atom; A.ft_ptr = flex->ftor_ptr; A.ft_bc = flex->ftor_bc;
    A.turn_ptr = flex->turn_ptr; A.turn = flex->turn; A.excl_ptr = flex->excl_ptr; A.excl = flex->excl;
    Q.best_rec = fo->best_rec; Q.cur_rec = fo->cur_rec; Q.q_flex_out = fo->q_flex_out;
    Q.NA = (size_t)B->NA; Q.NFT = (size_t)flex->n_ftor;
    // (the LDS attribute is set on every launch: it is per device, and a process may drive several)
    const size_t lds = sizeof(VinaSearchShared<V_FLEX_MAX_TOR>);
    if (dbfr_launch_check(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_vina_search<V_FLEX_MAX_TOR>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                          "k_vina_search<flex>: hipFuncSetAttribute(MaxDynamicSharedMemorySize)"))
      return dbfr_take_launch_error();
    hipLaunchKernelGGL(k_vina_search<V_FLEX_MAX_TOR>, grid, dim3(V_THREADS), lds, (hipStream_t)hip_stream, A, Q);
  } else {
    hipLaunchKernelGGL(k_vina_search<V_MAX_TOR>, grid, dim3(V_THREADS), 0, (hipStream_t)hip_stream, A, Q);
  }
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

extern "C" int dbfr_vina_search(const dbfr_vina_in* in, const dbfr_vina_opts* opts, const dbfr_vina_search_opts* search_opts,
                                const int64_t* stream, float* best_pos, float* cur_pos, float* terms, int32_t* iters, int32_t* accepted,
                                float* log, void* workspace, size_t workspace_bytes, void* hip_stream) {
  return vina_search_launch("dbfr_vina_search", in, opts, search_opts, stream, best_pos, cur_pos, terms, iters, accepted, log, workspace,
                            workspace_bytes, hip_stream);
}

extern "C" int dbfr_vina_flex_search_workspace_bytes(const dbfr_vina_flex_in* in, int32_t chains, size_t* bytes) {
  if (!in || !in->base) { dbfr_set_error("dbfr_vina_flex: null argument"); return DBFR_ERR_ARG; }
  size_t cap;
  const int rc = vina_search_check(in->base, chains, &cap, in);
  if (rc) return rc;
  if (!bytes) { dbfr_set_error("dbfr_vina_flex_search_workspace_bytes: null argument"); return DBFR_ERR_ARG; }
  *bytes = (size_t)chains * in->base->batch->G * cap * sizeof(float4);
  return DBFR_OK;
}

extern "C" int dbfr_vina_flex_search(const dbfr_vina_flex_in* in, const dbfr_vina_opts* opts, const dbfr_vina_search_opts* search_opts,
                                     const int64_t* stream, float* best_pos, float* best_rec, float* q_flex_out, float* cur_pos,
                                     float* cur_rec, float* terms, int32_t* iters, int32_t* accepted, float* log, void* workspace,
                                     size_t workspace_bytes, void* hip_stream) {
  if (!in || !in->base) { dbfr_set_error("dbfr_vina_flex: null argument"); return DBFR_ERR_ARG; }
  const VinaSearchFlexOut fo = {best_rec, q_flex_out, cur_rec};
  return vina_search_launch("dbfr_vina_flex_search", in->base, opts, search_opts, stream, best_pos, cur_pos, terms, iters, accepted, log,
                            workspace, workspace_bytes, hip_stream, in, &fo);
}

extern "C" int dbfr_vina_flex_workspace_bytes(const dbfr_vina_flex_in* in, size_t* bytes) {
  size_t cap;
  int rc = vina_flex_check(in, &cap);
  if (rc) return rc;
  if (!bytes) { dbfr_set_error("dbfr_vina_flex_workspace_bytes: null argument"); return DBFR_ERR_ARG; }
  *bytes = (size_t)in->base->batch->G * cap * sizeof(float4);
  return DBFR_OK;
}

extern "C" int dbfr_vina_flex_score_at(const dbfr_vina_flex_in* in, const float* q_rigid, const float* q_tor, const float* q_flex,
                                       float* lig_pos_out, float* rec_pos_out, float* terms, float* grad_rigid, float* grad_tor,
                                       float* grad_flex, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!in || !in->base) { dbfr_set_error("dbfr_vina_flex: null argument"); return DBFR_ERR_ARG; }
  const VinaFlexOut fo = {q_flex, rec_pos_out, nullptr, grad_flex};
  return vina_launch(in->base, 0, nullptr, q_rigid, q_tor, lig_pos_out, terms, grad_rigid, grad_tor, nullptr, workspace, workspace_bytes,
                     hip_stream, in, &fo);
}

extern "C" int dbfr_vina_flex_minimize(const dbfr_vina_flex_in* in, const dbfr_vina_opts* opts, float* lig_pos_out, float* rec_pos_out,
                                       float* q_flex_out, float* terms, int32_t* iters, void* workspace, size_t workspace_bytes,
                                       void* hip_stream) {
  if (!in || !in->base) { dbfr_set_error("dbfr_vina_flex: null argument"); return DBFR_ERR_ARG; }
  const VinaFlexOut fo = {nullptr, rec_pos_out, q_flex_out, nullptr};
  return vina_launch(in->base, 1, opts, nullptr, nullptr, lig_pos_out, terms, nullptr, nullptr, iters, workspace, workspace_bytes, hip_stream,
                     in, &fo);
}
