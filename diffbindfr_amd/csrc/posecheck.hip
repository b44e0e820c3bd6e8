// PoseBusters-style physical validity checks of poses: ligand-receptor distances and clashes, the lattice volume overlap, the
// internal clashes and the double-bond geometry of every frame of a ragged batch, in one launch.  include/dbfr.h states the
// definitions; docs/posecheck.md the layout and the limits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/dbfr.h"
#include "common.h"
#include "frames.h"

// One workgroup per frame.  The ligand (positions, radii) and, per atom, the bit mask of the lower-index ligand atoms whose
// lattice spheres can share a point with its own are staged in LDS.  The receptor (pocket atoms of the frame, then the static
// atoms of the group) streams past in tiles of one atom per thread: one pass gives d_min, rho, the clash count and, compacted
// in index order by ballot prefixes, the receptor atoms that can share a lattice point with some ligand atom.  The lattice
// pass walks every ligand atom's bounding box; a point inside the atom's sphere counts for the lowest-index atom whose sphere
// holds it (its neighbour mask says which atoms to ask) and is then tested against the compacted receptor atoms.  Every
// reduction is a min / max or an integer sum: the bits of a frame do not depend on the launch it is part of.
#define PC_THREADS FR_THREADS
#define PC_WAVES FR_WAVES
#define PC_MAX_LIG 256
#define PC_MAX_PAIR 32640          // every pair of 256 atoms
#define PC_MAX_FLAT 64
#define PC_MAX_STEREO 64
#define PC_FLAT_W 8                // fitted atoms per flatness bond (-1 padded)
#define PC_CAND 2048               // receptor candidates per frame kept in LDS (32 KB)
#define PC_MARGIN 0.01f            // A: candidate / neighbour filters are wider than the lattice test by this much

struct PcArgs {
  dbfr_pose_check_in in;
  dbfr_pose_check_opts o;
  dbfr_pose_check_out out;
  int cap;
};

__device__ __forceinline__ float dist2(float px, float py, float pz, float qx, float qy, float qz) {
  const float dx = px - qx, dy = py - qy, dz = pz - qz;
  return dx * dx + dy * dy + dz * dz;
}

// one Jacobi rotation of the symmetric 3x3 A zeroing A[p][q]; V accumulates the eigenvectors (columns)
template <int p, int q>
__device__ __forceinline__ void jacobi_rot(float (&A)[3][3], float (&V)[3][3]) {
  const float apq = A[p][q];
  if (apq == 0.f) return;
  const float theta = (A[q][q] - A[p][p]) / (2.f * apq);
  const float t = fabsf(theta) > 1e15f ? 0.5f / theta : copysignf(1.f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
  const float c = 1.f / sqrtf(t * t + 1.f), s = t * c;
  constexpr int r = 3 - p - q;
  const float arp = A[r][p], arq = A[r][q];
  A[r][p] = A[p][r] = c * arp - s * arq;
  A[r][q] = A[q][r] = s * arp + c * arq;
  A[p][p] -= t * apq;
  A[q][q] += t * apq;
  A[p][q] = A[q][p] = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float vp = V[k][p], vq = V[k][q];
    V[k][p] = c * vp - s * vq;
    V[k][q] = s * vp + c * vq;
  }
}

// largest distance of the points from their least-squares plane (normal = eigenvector of the smallest covariance eigenvalue)
__device__ float plane_dev(const float4* lx, const int* idx, int N) {
  float x[PC_FLAT_W][3];
  int n = 0;
  float cx = 0.f, cy = 0.f, cz = 0.f;
#pragma unroll
  for (int j = 0; j < PC_FLAT_W; ++j) {
    const int a = idx[j];
    const bool use = a >= 0;
    const float4 q = lx[use ? min(a, N - 1) : 0];
    x[j][0] = q.x; x[j][1] = q.y; x[j][2] = q.z;
    if (use) { cx += q.x; cy += q.y; cz += q.z; ++n; }
  }
  cx /= (float)n; cy /= (float)n; cz /= (float)n;
  float A[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  float V[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}};
#pragma unroll
  for (int j = 0; j < PC_FLAT_W; ++j) {
    if (idx[j] < 0) continue;
    const float d[3] = {x[j][0] - cx, x[j][1] - cy, x[j][2] - cz};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s = 0; s < 3; ++s) A[r][s] += d[r] * d[s];
  }
  for (int sweep = 0; sweep < 8; ++sweep) {
    jacobi_rot<0, 1>(A, V);
    jacobi_rot<0, 2>(A, V);
    jacobi_rot<1, 2>(A, V);
  }
  const int m = (A[0][0] <= A[1][1] && A[0][0] <= A[2][2]) ? 0 : (A[1][1] <= A[2][2] ? 1 : 2);
  const float nx = m == 0 ? V[0][0] : (m == 1 ? V[0][1] : V[0][2]);
  const float ny = m == 0 ? V[1][0] : (m == 1 ? V[1][1] : V[1][2]);
  const float nz = m == 0 ? V[2][0] : (m == 1 ? V[2][1] : V[2][2]);
  const float inv = 1.f / sqrtf(nx * nx + ny * ny + nz * nz);
  float dev = 0.f;
#pragma unroll
  for (int j = 0; j < PC_FLAT_W; ++j)
    if (idx[j] >= 0) dev = fmaxf(dev, fabsf(((x[j][0] - cx) * nx + (x[j][1] - cy) * ny + (x[j][2] - cz) * nz) * inv));
  return dev;
}

__global__ __launch_bounds__(PC_THREADS) void k_pose_check(PcArgs a) {
  __shared__ float4 lx[PC_MAX_LIG];                         // x, y, z, r
  __shared__ unsigned long long nbm[PC_MAX_LIG][4];         // bit c of atom a: c < a and their lattice spheres can meet
  __shared__ float4 cand[PC_CAND];                          // x, y, z, (vol_scale r)^2 of the receptor candidates
  __shared__ int wcnt[PC_WAVES];
  __shared__ float redf[PC_WAVES][4];
  __shared__ int redi[PC_WAVES][6];
  const dbfr_pose_check_in& in = a.in;
  const dbfr_pose_check_opts& o = a.o;
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = frame_group(in.frame_ptr, in.n_group, f);
  const int k = f - in.frame_ptr[g];
  const int l0 = in.lig_ptr[g], N = in.lig_ptr[g + 1] - l0;
  const int m0 = in.pocket_ptr[g], M = in.pocket_ptr[g + 1] - m0;
  const int s0 = in.static_ptr ? in.static_ptr[g] : 0, S = in.static_ptr ? in.static_ptr[g + 1] - s0 : 0;
  const int p0 = in.pair_ptr[g], NP = in.pair_ptr[g + 1] - p0;
  const int f0 = in.flat_ptr[g], NF = in.flat_ptr[g + 1] - f0;
  const int t0 = in.stereo_ptr[g], NST = in.stereo_ptr[g + 1] - t0;
  bool bad = N < 1 || N > in.max_lig || M < 0 || S < 0 || NP < 0 || NP > in.max_pair || NF < 0 || NF > in.max_flat ||
             NST < 0 || NST > in.max_stereo;
  const float vs = o.vol_scale, h = o.grid;
  int bad_atom = 0;
  if (!bad) {
    const float* lp = in.lig_pos + 3 * (in.lig_pos_off[g] + (long long)k * N);
    for (int i = tid; i < N; i += PC_THREADS) {
      const float x = lp[3 * i], y = lp[3 * i + 1], z = lp[3 * i + 2], r = in.lig_rad[l0 + i];
      bad_atom |= !atom_ok(x, y, z, r);
      lx[i] = make_float4(x, y, z, r);
    }
  }
  bad = __syncthreads_or(bad_atom) || bad;                  // uniform over the workgroup
  const dbfr_pose_check_out& out = a.out;
  if (bad) {                                                // counts outside the stated maxima or unusable atoms: NaN / -1
    if (tid == 0) {
      if (out.min_dist) out.min_dist[f] = NAN;
      if (out.min_ratio) out.min_ratio[f] = NAN;
      if (out.n_clash) out.n_clash[f] = -1;
      if (out.vol_lig) out.vol_lig[f] = -1;
      if (out.vol_overlap) out.vol_overlap[f] = -1;
      if (out.int_min_ratio) out.int_min_ratio[f] = NAN;
      if (out.n_int_clash) out.n_int_clash[f] = -1;
      if (out.flat_dev) out.flat_dev[f] = NAN;
      if (out.n_stereo_flip) out.n_stereo_flip[f] = -1;
      if (out.passed) out.passed[f] = 0;
    }
    return;
  }
  // neighbour masks of the lattice ownership test
  for (int t = tid; t < 4 * N; t += PC_THREADS) {
    const int i = t >> 2, w = t & 3;
    const float4 q = lx[i];
    const float Ri = vs * q.w;
    unsigned long long m = 0ull;
    for (int j = 0; j < 64; ++j) {
      const int c = w * 64 + j;
      if (c >= i) break;
      const float4 qc = lx[c];
      const float lim = Ri + vs * qc.w + PC_MARGIN;
      if (dist2(q.x, q.y, q.z, qc.x, qc.y, qc.z) < lim * lim) m |= 1ull << j;
    }
    nbm[i][w] = m;
  }
  // receptor pass: distances, ratios, clashes, candidates (index order: pocket atoms, then static atoms)
  const Receptor rec = {in.pocket_pos + 3 * (in.pocket_pos_off[g] + (long long)k * M), in.static_pos + 3 * (size_t)s0, in.pocket_rad + m0,
                        in.static_rad + s0, M};
  const int MR = M + S;
  float mind = INFINITY, minr = INFINITY;
  int ncl = 0, ncand = 0;
  for (int b0 = 0; b0 < MR; b0 += PC_THREADS) {
    const int b = b0 + tid;
    bool c = false;
    float yx = 0.f, yy = 0.f, yz = 0.f, rb = 0.f;
    if (b < MR) {
      const float* y = rec.pos(b);
      yx = y[0]; yy = y[1]; yz = y[2];
      rb = rec.rad(b);
      const float Rb = vs * rb;
      for (int i = 0; i < N; ++i) {
        const float4 q = lx[i];
        const float d = sqrtf(dist2(q.x, q.y, q.z, yx, yy, yz));
        const float ratio = d / (q.w + rb);
        mind = fminf(mind, d);
        minr = fminf(minr, ratio);
        ncl += ratio < o.clash_ratio;
        c = c || d < vs * q.w + Rb + PC_MARGIN;
      }
    }
    int slot, tot;
    block_compact(c, ncand, wcnt, lane, wave, slot, tot);
    if (c && slot < a.cap) {                                // a full list drops the entry: `spill` below sends the lattice pass to memory
      const float Rb = vs * rb;
      cand[slot] = make_float4(yx, yy, yz, Rb * Rb);
    }
    ncand += tot;
    __syncthreads();                                        // wcnt is rewritten by the next tile
  }
  const bool spill = ncand > a.cap;                         // uniform: the lattice pass reads every receptor atom instead
  // internal pairs
  float imin = INFINITY;
  int nic = 0;
  for (int t = tid; t < NP; t += PC_THREADS) {
    const int i = (int)min((unsigned)in.pair_ij[2 * (p0 + t)], (unsigned)(N - 1));
    const int j = (int)min((unsigned)in.pair_ij[2 * (p0 + t) + 1], (unsigned)(N - 1));
    const float4 qi = lx[i], qj = lx[j];
    const float ratio = sqrtf(dist2(qi.x, qi.y, qi.z, qj.x, qj.y, qj.z)) / (qi.w + qj.w);
    imin = fminf(imin, ratio);
    nic += ratio < o.internal_ratio;
  }
  // double bonds: flatness on wave 0, stereochemistry on wave 2
  float fdev = 0.f;
  int nflip = 0;
  if (tid < NF) {
    int idx[PC_FLAT_W];
#pragma unroll
    for (int j = 0; j < PC_FLAT_W; ++j) idx[j] = in.flat_atoms[(size_t)(f0 + tid) * PC_FLAT_W + j];
    fdev = plane_dev(lx, idx, N);
  }
  if (tid >= 128 && tid - 128 < NST) {
    const int t = t0 + tid - 128;
    float4 q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = lx[(int)min((unsigned)in.stereo_atoms[4 * t + j], (unsigned)(N - 1))];
    const float b1x = q[1].x - q[0].x, b1y = q[1].y - q[0].y, b1z = q[1].z - q[0].z;
    const float b2x = q[2].x - q[1].x, b2y = q[2].y - q[1].y, b2z = q[2].z - q[1].z;
    const float b3x = q[3].x - q[2].x, b3y = q[3].y - q[2].y, b3z = q[3].z - q[2].z;
    const float n1x = b1y * b2z - b1z * b2y, n1y = b1z * b2x - b1x * b2z, n1z = b1x * b2y - b1y * b2x;
    const float n2x = b2y * b3z - b2z * b3y, n2y = b2z * b3x - b2x * b3z, n2z = b2x * b3y - b2y * b3x;
    const float dot = n1x * n2x + n1y * n2y + n1z * n2z;
    const int sgn = dot > 0.f ? 1 : (dot < 0.f ? -1 : 0);
    nflip = sgn != (int)in.stereo_sign[t];
  }
  __syncthreads();                                          // nbm and cand complete
  // lattice pass
  int nvl = 0, nov = 0;
  const int ncheck = spill ? 0 : ncand;
  for (int i = 0; i < N; ++i) {
    const float4 q = lx[i];
    const float Ri = vs * q.w, R2 = Ri * Ri;
    const int x0 = (int)floorf((q.x - Ri) / h), y0 = (int)floorf((q.y - Ri) / h), z0 = (int)floorf((q.z - Ri) / h);
    const int nx = (int)ceilf((q.x + Ri) / h) - x0 + 1, ny = (int)ceilf((q.y + Ri) / h) - y0 + 1,
              nz = (int)ceilf((q.z + Ri) / h) - z0 + 1;
    const int B = nx * ny * nz;
    for (int t = tid; t < B; t += PC_THREADS) {
      const int ix = t % nx, iy = (t / nx) % ny, iz = t / (nx * ny);
      const float px = (float)(x0 + ix) * h, py = (float)(y0 + iy) * h, pz = (float)(z0 + iz) * h;
      if (!(dist2(px, py, pz, q.x, q.y, q.z) < R2)) continue;
      bool owned = true;
      for (int w = 0; w < 4 && owned; ++w) {
        unsigned long long m = nbm[i][w];
        while (m) {
          const int c = w * 64 + __ffsll((long long)m) - 1;
          m &= m - 1ull;
          const float4 qc = lx[c];
          const float Rc = vs * qc.w;
          if (dist2(px, py, pz, qc.x, qc.y, qc.z) < Rc * Rc) { owned = false; break; }
        }
      }
      if (!owned) continue;
      ++nvl;
      bool hit = false;
      for (int j = 0; j < ncheck && !hit; ++j) {
        const float4 cb = cand[j];
        hit = dist2(px, py, pz, cb.x, cb.y, cb.z) < cb.w;
      }
      if (spill)
        for (int b = 0; b < MR && !hit; ++b) {
          const float* y = rec.pos(b);
          const float Rb = vs * rec.rad(b);
          hit = dist2(px, py, pz, y[0], y[1], y[2]) < Rb * Rb;
        }
      nov += hit;
    }
  }
  // reductions: minima / maxima / integer sums, exact in any order
  mind = wave_min(mind);
  minr = wave_min(minr);
  imin = wave_min(imin);
  fdev = wave_max(fdev);
  ncl = wave_sum(ncl);
  nic = wave_sum(nic);
  nflip = wave_sum(nflip);
  nvl = wave_sum(nvl);
  nov = wave_sum(nov);
  if (lane == 0) {
    redf[wave][0] = mind; redf[wave][1] = minr; redf[wave][2] = imin; redf[wave][3] = fdev;
    redi[wave][0] = ncl; redi[wave][1] = nic; redi[wave][2] = nflip; redi[wave][3] = nvl; redi[wave][4] = nov;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < PC_WAVES; ++w) {
      mind = fminf(mind, redf[w][0]);
      minr = fminf(minr, redf[w][1]);
      imin = fminf(imin, redf[w][2]);
      fdev = fmaxf(fdev, redf[w][3]);
      ncl += redi[w][0];
      nic += redi[w][1];
      nflip += redi[w][2];
      nvl += redi[w][3];
      nov += redi[w][4];
    }
    int pass = 0;
    pass |= (minr >= o.clash_ratio) << 0;
    pass |= (mind <= o.max_distance) << 1;
    pass |= ((double)nov <= (double)o.vol_overlap * (double)nvl) << 2;
    pass |= (imin >= o.internal_ratio) << 3;
    pass |= (fdev <= o.flat_tol) << 4;
    pass |= (nflip == 0) << 5;
    pass |= (pass == 63) << 6;
    if (out.min_dist) out.min_dist[f] = mind;
    if (out.min_ratio) out.min_ratio[f] = minr;
    if (out.n_clash) out.n_clash[f] = ncl;
    if (out.vol_lig) out.vol_lig[f] = nvl;
    if (out.vol_overlap) out.vol_overlap[f] = nov;
    if (out.int_min_ratio) out.int_min_ratio[f] = imin;
    if (out.n_int_clash) out.n_int_clash[f] = nic;
    if (out.flat_dev) out.flat_dev[f] = fdev;
    if (out.n_stereo_flip) out.n_stereo_flip[f] = nflip;
    if (out.passed) out.passed[f] = pass;
  }
}

// ------------------------------------------------------------------------------------------------ host
extern "C" int dbfr_pose_check(const dbfr_pose_check_in* in, const dbfr_pose_check_opts* opts, const dbfr_pose_check_out* out,
                               void* hip_stream) {
  const char* fn = "dbfr_pose_check";
  if (!in || !out) return arg_err(fn, "null argument");
  if (in->n_group < 0 || in->n_frame < 0) return arg_err(fn, "negative n_group / n_frame");
  if (in->max_lig < 0 || in->max_lig > PC_MAX_LIG) return limit_err(fn, "max_lig (ligand atoms)", in->max_lig, 0, PC_MAX_LIG);
  if (in->max_pair < 0 || in->max_pair > PC_MAX_PAIR) return limit_err(fn, "max_pair (internal pairs)", in->max_pair, 0, PC_MAX_PAIR);
  if (in->max_flat < 0 || in->max_flat > PC_MAX_FLAT) return limit_err(fn, "max_flat (flatness bonds)", in->max_flat, 0, PC_MAX_FLAT);
  if (in->max_stereo < 0 || in->max_stereo > PC_MAX_STEREO) return limit_err(fn, "max_stereo (stereo bonds)", in->max_stereo, 0, PC_MAX_STEREO);
  if (in->cand_cap < 0 || in->cand_cap > PC_CAND) return limit_err(fn, "cand_cap (LDS receptor candidates)", in->cand_cap, 0, PC_CAND);
  dbfr_pose_check_opts o = {0.75f, 5.0f, 0.8f, 0.075f, 0.7f, 0.25f, 0.25f};
  if (opts) o = *opts;
  if (!(o.grid >= 0.05f && o.grid <= 1.f)) return arg_err(fn, "grid must lie in [0.05, 1] A");
  if (!(o.vol_scale > 0.f && o.vol_scale <= 2.f)) return arg_err(fn, "vol_scale must lie in (0, 2]");
  if (std::isnan(o.clash_ratio) || std::isnan(o.max_distance) || std::isnan(o.vol_overlap) || std::isnan(o.internal_ratio) ||
      std::isnan(o.flat_tol))
    return arg_err(fn, "a threshold is NaN");
  if (in->n_frame == 0) return DBFR_OK;
  if (in->n_group == 0) return arg_err(fn, "frames without groups");
  if (!in->frame_ptr || !in->lig_ptr || !in->lig_pos_off || !in->lig_pos || !in->lig_rad || !in->pocket_ptr ||
      !in->pocket_pos_off || !in->pair_ptr || !in->flat_ptr || !in->stereo_ptr)
    return arg_err(fn, "frame_ptr / lig_ptr / lig_pos_off / lig_pos / lig_rad / pocket_ptr / pocket_pos_off / pair_ptr / flat_ptr / "
                       "stereo_ptr missing");
  if (in->static_ptr && (!in->static_pos || !in->static_rad)) return arg_err(fn, "static_ptr given without static_pos / static_rad");
  PcArgs a;
  a.in = *in;
  a.o = o;
  a.out = *out;
  a.cap = in->cand_cap ? in->cand_cap : PC_CAND;
  HIPCHECK(launch_frames(k_pose_check, in->n_frame, PC_THREADS, 0, hip_stream, a));
  return DBFR_OK;
}
