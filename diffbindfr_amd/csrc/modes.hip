// Distinct binding modes of sampled poses: all-pairs symmetry-corrected RMSD within every group of poses (one ligand in one
// pocket frame) and the greedy mode selection / clustering on top of it.  include/dbfr.h states the definitions; docs/modes.md
// the layout and the limits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/dbfr.h"
#include "common.h"

// ------------------------------------------------------------------------------------------------ device: RMSD matrix
// Grid (tile, group).  A group's poses are cut into tiles of TB rows; the workgroup of tile pair (bi, bj), bi <= bj, stages the
// rows of both tiles in LDS (one copy when bi == bj) and computes every pair i < j between them.  Two ways to spread the pairs:
//   lane path: a lane per pose pair, the automorphisms in a loop (the perm row and the heavy flags are the same for every lane
//              of the wave: scalar loads);
//   wave path: a wave per pose pair, lanes over the automorphisms, then a wave minimum (groups of 32 automorphisms and more).
// Both compute every (pair, automorphism) mean square as ONE serial sum over the atoms in index order, so the bits of a group's
// matrix depend neither on the path, nor on the tile size, nor on the other groups of the launch (minima are exact).
#define MD_THREADS 256
#define MD_LDS_FLOATS 12288      // pose coordinates per workgroup (48 KB)
#define MD_MAX_TILE 64           // poses per tile: <= 2016 pairs in a diagonal tile, 4096 in the others
#define MD_MAX_POSE 4096
#define MD_MAX_ATOM 1024
#define MD_WAVE_PERMS 32         // from here on: the wave path

struct MdArgs {
  dbfr_pose_rmsd_in in;
  float* out;
  int tb;                        // poses per tile
};

// sums over h < g of {P_h N_h, n_perm_h N_h, P_h^2}: where group g's positions, perms and matrix start (integers: exact in any order)
__device__ void group_offsets(const dbfr_pose_rmsd_in& in, int g, long long* off) {
  __shared__ long long red[MD_THREADS / 64][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long s0 = 0, s1 = 0, s2 = 0;
  for (int h = tid; h < g; h += MD_THREADS) {
    const long long P = in.pose_ptr[h + 1] - in.pose_ptr[h], N = in.atom_ptr[h + 1] - in.atom_ptr[h],
                    Q = in.perm_ptr ? in.perm_ptr[h + 1] - in.perm_ptr[h] : 0;
    s0 += P * N;
    s1 += Q * N;
    s2 += P * P;
  }
  for (int o = 32; o > 0; o >>= 1) {
    s0 += __shfl_xor(s0, o);
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  if (lane == 0) { red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; }
  __syncthreads();
  for (int k = 0; k < 3; ++k) {
    long long s = 0;
    for (int w = 0; w < MD_THREADS / 64; ++w) s += red[w][k];
    off[k] = s;
  }
  __syncthreads();
}

// mean square distance of pose xi under the automorphism perm to pose xj, over the heavy atoms (hv NULL: all), then the root
__device__ __forceinline__ float perm_rmsd(const float* xi, const float* xj, const int* perm, const int* hv, int n) {
  float acc = 0.f, cnt = 0.f;
  for (int a = 0; a < n; ++a) {
    const int s = (int)min((unsigned)perm[a], (unsigned)(n - 1));     // a malformed perm cannot leave the group's rows
    if (!hv || (hv[a] && hv[s])) {
      const float dx = xi[3 * s] - xj[3 * a], dy = xi[3 * s + 1] - xj[3 * a + 1], dz = xi[3 * s + 2] - xj[3 * a + 2];
      acc += dx * dx + dy * dy + dz * dz;
      cnt += 1.f;
    }
  }
  return sqrtf(acc / cnt);
}

__global__ __launch_bounds__(MD_THREADS) void k_pose_rmsd(MdArgs a) {
  extern __shared__ float xs[];                        // tile bi rows, then tile bj rows (bi != bj)
  const dbfr_pose_rmsd_in& in = a.in;
  const int g = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = in.pose_ptr[g + 1] - in.pose_ptr[g], N = in.atom_ptr[g + 1] - in.atom_ptr[g],
            NP = in.perm_ptr[g + 1] - in.perm_ptr[g];
  if (P <= 0) return;
  const int TB = a.tb, T = (P + TB - 1) / TB;
  const bool bad = P > in.max_pose || N < 1 || N > in.max_atom || NP < 1;
  if (bad ? blockIdx.x > 0 : (int)blockIdx.x >= T * (T + 1) / 2) return;        // uniform over the workgroup
  long long off[3];
  group_offsets(in, g, off);
  float* out = a.out + off[2];
  if (bad) {                                            // counts outside the stated maxima: NaN, nothing else read
    for (long long k = tid; k < (long long)P * P; k += MD_THREADS) out[k] = NAN;
    return;
  }
  int bi = 0, t = blockIdx.x;                           // upper-triangle tile pair number t -> (bi, bj)
  while (t >= T - bi) { t -= T - bi; ++bi; }
  const int bj = bi + t;
  const int r0 = bi * TB, c0 = bj * TB, ni = min(TB, P - r0), nj = min(TB, P - c0), n3 = 3 * N;
  const float* src = in.pos + 3 * off[0];
  float* xi = xs;
  float* xj = bi == bj ? xs : xs + ni * n3;
  for (int k = tid; k < ni * n3; k += MD_THREADS) xi[k] = src[(size_t)r0 * n3 + k];
  if (bi != bj)
    for (int k = tid; k < nj * n3; k += MD_THREADS) xj[k] = src[(size_t)c0 * n3 + k];
  __syncthreads();
  const int* perms = in.perms + off[1];
  const int* hv = in.heavy_mask ? in.heavy_mask + in.atom_ptr[g] : nullptr;
  const int npairs = bi == bj ? ni * (ni - 1) / 2 : ni * nj;
  const bool wave_path = in.path == 2 || (in.path == 0 && NP >= MD_WAVE_PERMS);
  if (bi == bj)
    for (int r = tid; r < ni; r += MD_THREADS) out[(size_t)(r0 + r) * P + r0 + r] = 0.f;
  const int k0 = wave_path ? wave : tid, kstep = wave_path ? MD_THREADS / 64 : MD_THREADS;
  for (int k = k0; k < npairs; k += kstep) {
    int r, c;
    if (bi == bj) {                                     // k -> (r, c), r < c: row r holds ni - 1 - r pairs
      r = 0;
      int kk = k;
      while (kk >= ni - 1 - r) { kk -= ni - 1 - r; ++r; }
      c = r + 1 + kk;
    } else {
      r = k / nj;
      c = k - r * nj;
    }
    const float* pi = xi + r * n3;
    const float* pj = xj + c * n3;
    float best = INFINITY;
    if (wave_path) {
      for (int p = lane; p < NP; p += 64) best = fminf(best, perm_rmsd(pi, pj, perms + (size_t)p * N, hv, N));
      for (int o = 32; o > 0; o >>= 1) best = fminf(best, __shfl_xor(best, o));
      if (lane != 0) continue;
    } else {
      for (int p = 0; p < NP; ++p) best = fminf(best, perm_rmsd(pi, pj, perms + (size_t)p * N, hv, N));
    }
    const int i = r0 + r, j = c0 + c;
    out[(size_t)i * P + j] = best;
    out[(size_t)j * P + i] = best;
  }
}

// ------------------------------------------------------------------------------------------------ device: mode selection
// One workgroup per group: every thread ranks poses by counting the ones that sort before them (O(P^2) compares, no sort
// network to get wrong), wave 0 walks the order and keeps the modes, then every thread assigns poses and counts clusters.
struct SmArgs {
  dbfr_pose_rmsd_in in;
  const float* rmsd;
  const float* score;
  dbfr_modes_opts o;
  int32_t *mode_rank, *mode_id, *cluster_size;
};

__global__ __launch_bounds__(MD_THREADS) void k_select_modes(SmArgs a) {
  __shared__ float key[MD_MAX_POSE];                   // score, negated when higher is better: lower key = better
  __shared__ int ord[MD_MAX_POSE];                     // poses in key order; after the walk: the cluster of every pose
  __shared__ int kept[MD_MAX_POSE];                    // kept modes by rank
  __shared__ int n_kept;
  const dbfr_pose_rmsd_in& in = a.in;
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p0 = in.pose_ptr[g], P = in.pose_ptr[g + 1] - p0;
  if (P <= 0) return;
  if (P > in.max_pose) {
    for (int i = tid; i < P; i += MD_THREADS) { a.mode_rank[p0 + i] = -1; a.mode_id[p0 + i] = -1; a.cluster_size[p0 + i] = 0; }
    return;
  }
  long long off[3];
  group_offsets(in, g, off);
  const float* R = a.rmsd + off[2];
  for (int i = tid; i < P; i += MD_THREADS) {
    const float s = a.score[p0 + i];
    key[i] = a.o.higher_is_better ? -s : s;
  }
  __syncthreads();
  for (int i = tid; i < P; i += MD_THREADS) {
    const float ki = key[i];
    const bool ni = isnan(ki);
    int rank = 0;
    for (int k = 0; k < P; ++k) {
      const float kk = key[k];
      const bool nk = isnan(kk);
      rank += ni ? (!nk || k < i) : (!nk && (kk < ki || (kk == ki && k < i)));
    }
    ord[rank] = i;
  }
  __syncthreads();
  if (wave == 0) {
    const float best = key[ord[0]];
    const bool use_range = a.o.energy_range >= 0.f;
    int nm = 0;
    for (int t = 0; t < P; ++t) {
      const int c = ord[t];
      const float s = key[c];
      if (isnan(s) || (use_range && !(s <= best + a.o.energy_range))) break;       // sorted: nothing behind qualifies either
      bool ok = true;
      for (int m = lane; m < nm; m += 64) ok = ok && R[(size_t)kept[m] * P + c] >= a.o.min_rmsd;
      if (__any(!ok)) continue;
      kept[nm] = c;                                     // every lane writes it, and reads back only entries it wrote itself
      ++nm;
      if (a.o.num_modes > 0 && nm == a.o.num_modes) break;
    }
    if (lane == 0) n_kept = nm;
  }
  __syncthreads();
  const int nm = n_kept;
  int* cid = ord;
  for (int i = tid; i < P; i += MD_THREADS) {
    float best = INFINITY;
    int id = -1;
    for (int m = 0; m < nm; ++m) {                      // rank order: a tie stays with the better-ranked mode
      const float r = R[(size_t)kept[m] * P + i];     // = R[i, mode] (the matrix is mirrored bitwise)
      if (r < best) { best = r; id = m; }
    }
    if (!(best <= a.o.cluster_rmsd)) id = -1;
    cid[i] = id;
    a.mode_id[p0 + i] = id;
    a.mode_rank[p0 + i] = (id >= 0 && kept[id] == i) ? id : -1;
  }
  __syncthreads();
  for (int r = tid; r < P; r += MD_THREADS) {
    int cnt = 0;
    if (r < nm)
      for (int i = 0; i < P; ++i) cnt += cid[i] == r;
    a.cluster_size[p0 + r] = cnt;
  }
}

// ------------------------------------------------------------------------------------------------ host
static int rmsd_in_check(const dbfr_pose_rmsd_in* in, const char* fn) {
  const std::string f = std::string(fn) + ": ";
  if (!in) { dbfr_set_error(f + "null argument"); return DBFR_ERR_ARG; }
  if (in->n_group < 0) { dbfr_set_error(f + "negative n_group"); return DBFR_ERR_ARG; }
  if (in->n_group > 0 && !in->pose_ptr) { dbfr_set_error(f + "pose_ptr missing"); return DBFR_ERR_ARG; }
  if (in->max_pose < 0 || in->max_pose > MD_MAX_POSE) {
    dbfr_set_error(f + "max_pose " + std::to_string(in->max_pose) + " outside [0, " + std::to_string(MD_MAX_POSE) + "]: groups of more than " +
                   std::to_string(MD_MAX_POSE) + " poses are not supported");
    return DBFR_ERR_ARG;
  }
  if (in->n_group > 65535) { dbfr_set_error(f + "more than 65535 groups in one launch"); return DBFR_ERR_ARG; }
  return DBFR_OK;
}

extern "C" int dbfr_pose_rmsd_matrix(const dbfr_pose_rmsd_in* in, float* rmsd_out, void* hip_stream) {
  if (int rc = rmsd_in_check(in, "dbfr_pose_rmsd_matrix")) return rc;
  if (in->n_group == 0 || in->max_pose == 0) return DBFR_OK;
  if (in->max_atom < 1 || in->max_atom > MD_MAX_ATOM) {
    dbfr_set_error("dbfr_pose_rmsd_matrix: max_atom " + std::to_string(in->max_atom) + " outside [1, " + std::to_string(MD_MAX_ATOM) + "]");
    return DBFR_ERR_ARG;
  }
  if (!in->atom_ptr || !in->perm_ptr || !in->pos || !in->perms || !rmsd_out) {
    dbfr_set_error("dbfr_pose_rmsd_matrix: atom_ptr / perm_ptr / pos / perms / rmsd_out missing");
    return DBFR_ERR_ARG;
  }
  if (in->path < 0 || in->path > 2) { dbfr_set_error("dbfr_pose_rmsd_matrix: path must be 0, 1 or 2"); return DBFR_ERR_ARG; }
  if (in->tile_rows < 0) { dbfr_set_error("dbfr_pose_rmsd_matrix: negative tile_rows"); return DBFR_ERR_ARG; }
  const int n3 = 3 * in->max_atom;
  int tb;
  if (in->max_pose <= MD_MAX_TILE && in->max_pose * n3 <= MD_LDS_FLOATS) tb = in->max_pose;       // a group is one tile
  else tb = std::max(1, std::min(MD_MAX_TILE, MD_LDS_FLOATS / (2 * n3)));
  if (in->tile_rows > 0) tb = std::min(tb, in->tile_rows);
  const int T = (in->max_pose + tb - 1) / tb;
  const int lds = (T == 1 ? 1 : 2) * tb * n3 * (int)sizeof(float);
  MdArgs a;
  a.in = *in;
  a.out = rmsd_out;
  a.tb = tb;
  hipLaunchKernelGGL(k_pose_rmsd, dim3((unsigned)(T * (T + 1) / 2), (unsigned)in->n_group), dim3(MD_THREADS), lds,
                     (hipStream_t)hip_stream, a);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

extern "C" int dbfr_select_modes(const dbfr_pose_rmsd_in* in, const float* rmsd, const float* score, const dbfr_modes_opts* opts,
                                 int32_t* mode_rank, int32_t* mode_id, int32_t* cluster_size, void* hip_stream) {
  if (int rc = rmsd_in_check(in, "dbfr_select_modes")) return rc;
  dbfr_modes_opts o = {9, 0, 1.0f, 2.0f, -1.0f};
  if (opts) o = *opts;
  if (o.num_modes < 0) { dbfr_set_error("dbfr_select_modes: negative num_modes"); return DBFR_ERR_ARG; }
  if (o.higher_is_better != 0 && o.higher_is_better != 1) { dbfr_set_error("dbfr_select_modes: higher_is_better must be 0 or 1"); return DBFR_ERR_ARG; }
  if (!(o.min_rmsd > 0.f) || !std::isfinite(o.min_rmsd)) { dbfr_set_error("dbfr_select_modes: min_rmsd must be finite and > 0"); return DBFR_ERR_ARG; }
  if (!(o.cluster_rmsd >= o.min_rmsd)) { dbfr_set_error("dbfr_select_modes: cluster_rmsd must be >= min_rmsd"); return DBFR_ERR_ARG; }
  if (std::isnan(o.energy_range)) { dbfr_set_error("dbfr_select_modes: energy_range is NaN (< 0 = off)"); return DBFR_ERR_ARG; }
  if (o.energy_range >= 0.f && o.higher_is_better) {
    dbfr_set_error("dbfr_select_modes: energy_range applies to lower-is-better scores only");
    return DBFR_ERR_ARG;
  }
  if (in->n_group == 0 || in->max_pose == 0) return DBFR_OK;
  if (!rmsd || !score || !mode_rank || !mode_id || !cluster_size) {
    dbfr_set_error("dbfr_select_modes: rmsd / score / mode_rank / mode_id / cluster_size missing");
    return DBFR_ERR_ARG;
  }
  SmArgs a;
  a.in = *in;
  a.in.atom_ptr = in->pose_ptr;                         // group_offsets reads them; only the P_h^2 sum is used here
  a.in.perm_ptr = nullptr;
  a.rmsd = rmsd;
  a.score = score;
  a.o = o;
  a.mode_rank = mode_rank;
  a.mode_id = mode_id;
  a.cluster_size = cluster_size;
  hipLaunchKernelGGL(k_select_modes, dim3((unsigned)in->n_group), dim3(MD_THREADS), 0, (hipStream_t)hip_stream, a);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}
