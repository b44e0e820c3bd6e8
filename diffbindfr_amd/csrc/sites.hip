// Binding-site detection in the LIGSITE style for a ragged batch of proteins: occupancy of the lattice h Z^3, burial along 7
// lines, pocket points, their 6-connected components, per-site integer sums, ranking and lining residues.  include/dbfr.h
// states the definitions; docs/sites.md the layout and the limits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/dbfr.h"
#include "common.h"

// The call's grids are concatenated (protein p's points at pt_off[p] ..).  Work per kernel:
//   k_sites_bounds   one workgroup per protein: min / max of its atoms (read back; the host sizes the grids)
//   k_sites_occ      one thread per atom: marks the lattice points of its sphere (every writer stores 1)
//   k_sites_burial   one thread per point: 7 lines x 2 senses of byte loads; per block the number of pocket points
//   k_sites_scan     one workgroup: exclusive scan of the block counts
//   k_sites_compact  the pocket points in grid order (ballot prefixes), so compact order = linear-index order per protein
//   k_sites_union    one thread per pocket point: union with its +x / +y / +z pocket neighbours; a root is only ever hooked
//                    under a SMALLER root (atomicCAS), so every component ends at its smallest compact index = smallest label
//   k_sites_reduce   root of every point; n_points / score / idx_sum by int32 / int64 atomics at the root
//   k_sites_rank     one workgroup per protein: the max_sites best roots by (score, -label), one block max per site
//   k_sites_lining   one thread per atom: the points of the kept sites within lining_cutoff
// Every result is an integer sum, a min-label or a max: a protein's bits do not depend on the launch it is part of.
#define ST_THREADS 256
#define ST_MAX_AXIS 1024
#define ST_MAX_PROT_POINTS (1 << 24)
#define ST_MAX_POINTS (1ll << 30)
#define ST_MAX_SITES 64

struct StGrid {
  int lo[3];
  int n[3];
};

struct StArgs {
  dbfr_sites_in in;
  dbfr_sites_out out;
  float h, probe, cut;
  int min_b, min_pts, S;
  int tax, tdg;                    // steps along an axis / a body diagonal
  int total;                       // grid points of the call
  int nblk;                        // burial blocks
  const StGrid* grid;              // [P]
  const int* pt_off;               // [P + 1]
  float* bounds;                   // [P, 6]
  uint8_t* occ;
  uint8_t* bur;
  int* blk;                        // [nblk + 1] counts, then exclusive offsets (blk[nblk] = pocket points)
  int* list;                       // [total] global point index of pocket point v
  int* parent;                     // [total]
  int* cnt;                        // [total]
  int* score;                      // [total]
  unsigned long long* sums;        // [total, 3]
  int* slot;                       // [total] site slot of a kept root, else -1
  int* kr;                         // [P, 2] compact range of every protein
};

// last p with ptr[p] <= x (ptr ascending, ptr[0] <= x < ptr[n])
__device__ __forceinline__ int seg_of(const int* ptr, int n, int x) {
  int a = 0, b = n;                // invariant: ptr[a] <= x < ptr[b]
  while (b - a > 1) {
    const int m = (a + b) >> 1;
    if (ptr[m] <= x) a = m; else b = m;
  }
  return a;
}

// first v in [a, b) with list[v] >= x
__device__ __forceinline__ int lower_bound(const int* list, int a, int b, int x) {
  while (a < b) {
    const int m = (a + b) >> 1;
    if (list[m] < x) a = m + 1; else b = m;
  }
  return a;
}

__device__ __forceinline__ bool is_pocket(const StArgs& a, int g) { return !a.occ[g] && a.bur[g] >= a.min_b; }

__device__ __forceinline__ int find_root(int* parent, int v) {
  int p = __atomic_load_n(&parent[v], __ATOMIC_RELAXED);
  while (p != v) {
    const int gp = __atomic_load_n(&parent[p], __ATOMIC_RELAXED);
    if (gp != p) __atomic_store_n(&parent[v], gp, __ATOMIC_RELAXED);      // path halving: gp is an ancestor of v
    v = p;
    p = gp;
  }
  return v;
}

// ------------------------------------------------------------------------------------------------ kernels
__global__ void __launch_bounds__(ST_THREADS) k_sites_bounds(StArgs a) {
  const int p = blockIdx.x;
  const int r0 = a.in.res_ptr[p], r1 = a.in.res_ptr[p + 1];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int t = r0 * 37 + threadIdx.x; t < r1 * 37; t += ST_THREADS) {
    if (!(a.in.atom37_mask[t] > 0.f)) continue;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float x = a.in.atom37_pos[3 * (size_t)t + d];
      mn[d] = fminf(mn[d], x);
      mx[d] = fmaxf(mx[d], x);
    }
  }
  __shared__ float red[6][ST_THREADS / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    for (int o = 32; o > 0; o >>= 1) {
      mn[d] = fminf(mn[d], __shfl_xor(mn[d], o));
      mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], o));
    }
    if (lane == 0) { red[d][w] = mn[d]; red[3 + d][w] = mx[d]; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = red[threadIdx.x][0];
    for (int k = 1; k < ST_THREADS / 64; ++k) v = threadIdx.x < 3 ? fminf(v, red[threadIdx.x][k]) : fmaxf(v, red[threadIdx.x][k]);
    a.bounds[6 * p + threadIdx.x] = v;
  }
}

__global__ void __launch_bounds__(ST_THREADS) k_sites_occ(StArgs a) {
  const int t = blockIdx.x * ST_THREADS + threadIdx.x;
  if (t >= a.in.n_res * 37 || !(a.in.atom37_mask[t] > 0.f)) return;
  const int res = t / 37, p = seg_of(a.in.res_ptr, a.in.n_prot, res);
  const StGrid G = a.grid[p];
  int aa = a.in.aatype[res];
  if (aa < 0 || aa > 20) aa = 20;
  const float R = a.in.radius[aa * 37 + t % 37] + a.probe;
  const float R2 = R * R;
  float x[3];
  int b0[3], b1[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    x[d] = a.in.atom37_pos[3 * (size_t)t + d];
    b0[d] = max((int)floorf((x[d] - R) / a.h) - 1, G.lo[d]) - G.lo[d];           // one point wider: the exact test decides
    b1[d] = min((int)floorf((x[d] + R) / a.h) + 1, G.lo[d] + G.n[d] - 1) - G.lo[d];
  }
  uint8_t* occ = a.occ + a.pt_off[p];
  for (int k = b0[2]; k <= b1[2]; ++k) {
    const float dz = a.h * (float)(G.lo[2] + k) - x[2];
    for (int j = b0[1]; j <= b1[1]; ++j) {
      const float dy = a.h * (float)(G.lo[1] + j) - x[1];
      for (int i = b0[0]; i <= b1[0]; ++i) {
        const float dx = a.h * (float)(G.lo[0] + i) - x[0];
        if (dx * dx + dy * dy + dz * dz < R2) occ[i + G.n[0] * (j + G.n[1] * k)] = 1;
      }
    }
  }
}

// does the walk from (i, j, k) along (di, dj, dk) reach an occupied point within T steps?
__device__ __forceinline__ bool ray_hits(const uint8_t* occ, const StGrid& G, int i, int j, int k, int di, int dj, int dk, int T) {
  for (int s = 1; s <= T; ++s) {
    i += di; j += dj; k += dk;
    if (i < 0 || j < 0 || k < 0 || i >= G.n[0] || j >= G.n[1] || k >= G.n[2]) return false;     // off the grid: solvent from here on
    if (occ[i + G.n[0] * (j + G.n[1] * k)]) return true;
  }
  return false;
}

__global__ void __launch_bounds__(ST_THREADS) k_sites_burial(StArgs a) {
  const int g = blockIdx.x * ST_THREADS + threadIdx.x;
  bool pocket = false;
  if (g < a.total) {
    const int p = seg_of(a.pt_off, a.in.n_prot, g);
    const StGrid G = a.grid[p];
    const uint8_t* occ = a.occ + a.pt_off[p];
    const int l = g - a.pt_off[p];
    const int i = l % G.n[0], j = (l / G.n[0]) % G.n[1], k = l / (G.n[0] * G.n[1]);
    int b = 0;
    if (!occ[l]) {
      const int dir[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {-1, 1, 1}};
#pragma unroll
      for (int e = 0; e < 7; ++e) {
        const int T = e < 3 ? a.tax : a.tdg;
        if (ray_hits(occ, G, i, j, k, dir[e][0], dir[e][1], dir[e][2], T) && ray_hits(occ, G, i, j, k, -dir[e][0], -dir[e][1], -dir[e][2], T))
          ++b;
      }
    }
    a.bur[g] = (uint8_t)b;
    pocket = b >= a.min_b;
  }
  const int n = __syncthreads_count(pocket);
  if (threadIdx.x == 0) a.blk[blockIdx.x] = n;
}

__global__ void __launch_bounds__(1024) k_sites_scan(StArgs a) {
  __shared__ int part[1024];
  const int per = (a.nblk + 1023) / 1024, b0 = threadIdx.x * per, b1 = min(b0 + per, a.nblk);
  int s = 0;
  for (int b = b0; b < b1; ++b) s += a.blk[b];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {                 // inclusive Hillis-Steele scan of the 1024 partial sums
    const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int run = part[threadIdx.x] - s;
  for (int b = b0; b < b1; ++b) {
    const int c = a.blk[b];
    a.blk[b] = run;
    run += c;
  }
  if (threadIdx.x == 1023) a.blk[a.nblk] = part[1023];
}

__global__ void __launch_bounds__(ST_THREADS) k_sites_compact(StArgs a) {
  const int g = blockIdx.x * ST_THREADS + threadIdx.x;
  const bool pocket = g < a.total && is_pocket(a, g);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(pocket);
  __shared__ int wsum[ST_THREADS / 64];
  if (lane == 0) wsum[w] = __popcll(bal);
  __syncthreads();
  if (!pocket) return;
  int pos = a.blk[blockIdx.x] + __popcll(bal & ((1ull << lane) - 1ull));
  for (int k = 0; k < w; ++k) pos += wsum[k];
  a.list[pos] = g;
  a.parent[pos] = pos;
  a.cnt[pos] = 0;
  a.score[pos] = 0;
  a.sums[3 * (size_t)pos] = a.sums[3 * (size_t)pos + 1] = a.sums[3 * (size_t)pos + 2] = 0ull;
  a.slot[pos] = -1;
}

__global__ void __launch_bounds__(ST_THREADS) k_sites_union(StArgs a) {
  const int v = blockIdx.x * ST_THREADS + threadIdx.x;
  const int K = a.blk[a.nblk];
  if (v >= K) return;
  const int g = a.list[v];
  const int p = seg_of(a.pt_off, a.in.n_prot, g);
  const StGrid G = a.grid[p];
  const int l = g - a.pt_off[p];
  const int ijk[3] = {l % G.n[0], (l / G.n[0]) % G.n[1], l / (G.n[0] * G.n[1])};
  const int step[3] = {1, G.n[0], G.n[0] * G.n[1]};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (ijk[d] + 1 >= G.n[d] || !is_pocket(a, g + step[d])) continue;
    int u = lower_bound(a.list, v + 1, min(K, v + 1 + step[d]), g + step[d]);       // the neighbour's compact index
    int rv = find_root(a.parent, v), ru = find_root(a.parent, u);
    while (rv != ru) {                                  // hook the larger root under the smaller one
      if (rv < ru) {
        const int got = atomicCAS(&a.parent[ru], ru, rv);
        if (got == ru) break;
        ru = find_root(a.parent, got);
      } else {
        const int got = atomicCAS(&a.parent[rv], rv, ru);
        if (got == rv) break;
        rv = find_root(a.parent, got);
      }
    }
  }
}

__global__ void __launch_bounds__(ST_THREADS) k_sites_reduce(StArgs a) {
  const int v = blockIdx.x * ST_THREADS + threadIdx.x;
  const int K = a.blk[a.nblk];
  if (v >= K) return;
  int r = v, up;
  while ((up = __atomic_load_n(&a.parent[r], __ATOMIC_RELAXED)) != r) r = up;      // the forest is final: walk to the root
  const int g = a.list[v];
  const int p = seg_of(a.pt_off, a.in.n_prot, g);
  const StGrid G = a.grid[p];
  const int l = g - a.pt_off[p];
  atomicAdd(&a.cnt[r], 1);
  atomicAdd(&a.score[r], (int)a.bur[g]);
  atomicAdd(&a.sums[3 * (size_t)r], (unsigned long long)(l % G.n[0]));
  atomicAdd(&a.sums[3 * (size_t)r + 1], (unsigned long long)((l / G.n[0]) % G.n[1]));
  atomicAdd(&a.sums[3 * (size_t)r + 2], (unsigned long long)(l / (G.n[0] * G.n[1])));
  if (a.out.labels) a.out.labels[g] = a.list[r] - a.pt_off[p];
  __atomic_store_n(&a.parent[v], r, __ATOMIC_RELAXED);                        // (an ancestor: concurrent walks stay valid)
}

__global__ void __launch_bounds__(ST_THREADS) k_sites_rank(StArgs a) {
  const int p = blockIdx.x;
  const int K = a.blk[a.nblk];
  __shared__ int kr[2];
  __shared__ unsigned long long wbest[ST_THREADS / 64];
  __shared__ int nsel;
  if (threadIdx.x == 0) {
    kr[0] = lower_bound(a.list, 0, K, a.pt_off[p]);
    kr[1] = lower_bound(a.list, kr[0], K, a.pt_off[p + 1]);
    a.kr[2 * p] = kr[0];
    a.kr[2 * p + 1] = kr[1];
    nsel = 0;
  }
  __syncthreads();
  const int k0 = kr[0], k1 = kr[1], S = a.S, base = a.pt_off[p];
  const StGrid G = a.grid[p];
  unsigned long long prev = ~0ull;
  for (int s = 0; s < S; ++s) {
    // key = score << 32 | (2^32 - 1 - label): unique per root, larger = better
    unsigned long long best = 0ull;
    for (int v = k0 + threadIdx.x; v < k1; v += ST_THREADS) {
      if (a.parent[v] != v || a.cnt[v] < a.min_pts) continue;
      const unsigned long long key = ((unsigned long long)a.score[v] << 32) | (0xFFFFFFFFull - (unsigned)(a.list[v] - base));
      if (key < prev && key > best) best = key;
    }
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(best, o);
      best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
    __syncthreads();
    best = wbest[0];
    for (int k = 1; k < ST_THREADS / 64; ++k) best = wbest[k] > best ? wbest[k] : best;
    __syncthreads();
    if (best == 0ull) break;                            // (uniform) no further site
    prev = best;
    if (threadIdx.x == 0) {
      const int label = (int)(0xFFFFFFFFull - (best & 0xFFFFFFFFull));
      const int v = lower_bound(a.list, k0, k1, base + label);
      const int o = p * S + s;
      a.slot[v] = s;
      a.out.label[o] = label;
      a.out.n_points[o] = a.cnt[v];
      a.out.score[o] = a.score[v];
      for (int d = 0; d < 3; ++d) {
        const long long sum = (long long)a.sums[3 * (size_t)v + d];
        if (a.out.idx_sum) a.out.idx_sum[3 * o + d] = sum;
        a.out.centre[3 * o + d] = (double)a.h * ((double)G.lo[d] + (double)sum / (double)a.cnt[v]);
      }
      nsel = s + 1;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) a.out.n_sites[p] = nsel;
  for (int s = nsel + threadIdx.x; s < S; s += ST_THREADS) {
    const int o = p * S + s;
    a.out.label[o] = -1;
    a.out.n_points[o] = 0;
    a.out.score[o] = 0;
    for (int d = 0; d < 3; ++d) {
      if (a.out.idx_sum) a.out.idx_sum[3 * o + d] = 0;
      a.out.centre[3 * o + d] = 0.0;
    }
  }
}

__global__ void __launch_bounds__(ST_THREADS) k_sites_lining(StArgs a) {
  const int t = blockIdx.x * ST_THREADS + threadIdx.x;
  if (t >= a.in.n_res * 37 || !(a.in.atom37_mask[t] > 0.f)) return;
  const int res = t / 37, p = seg_of(a.in.res_ptr, a.in.n_prot, res);
  if (a.out.n_sites[p] == 0) return;
  const StGrid G = a.grid[p];
  const int base = a.pt_off[p], k0 = a.kr[2 * p], k1 = a.kr[2 * p + 1];
  const float c2 = a.cut * a.cut;
  float x[3];
  int b0[3], b1[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    x[d] = a.in.atom37_pos[3 * (size_t)t + d];
    b0[d] = max((int)floorf((x[d] - a.cut) / a.h) - 1, G.lo[d]) - G.lo[d];
    b1[d] = min((int)floorf((x[d] + a.cut) / a.h) + 1, G.lo[d] + G.n[d] - 1) - G.lo[d];
  }
  uint8_t* row = a.out.lining + (size_t)res * a.S;
  for (int k = b0[2]; k <= b1[2]; ++k) {
    const float dz = a.h * (float)(G.lo[2] + k) - x[2];
    for (int j = b0[1]; j <= b1[1]; ++j) {
      const float dy = a.h * (float)(G.lo[1] + j) - x[1];
      for (int i = b0[0]; i <= b1[0]; ++i) {
        const int g = base + i + G.n[0] * (j + G.n[1] * k);
        if (!is_pocket(a, g)) continue;
        const float dx = a.h * (float)(G.lo[0] + i) - x[0];
        if (!(dx * dx + dy * dy + dz * dz <= c2)) continue;
        const int s = a.slot[a.parent[lower_bound(a.list, k0, k1, g)]];
        if (s >= 0) row[s] = 1;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

struct StLayout {
  size_t bounds, grid, pt_off, kr, occ, bur, blk, list, parent, cnt, score, sums, slot, total;
};

static StLayout st_layout(int P, int64_t T) {
  StLayout L;
  const size_t nblk = (size_t)((T + ST_THREADS - 1) / ST_THREADS);
  size_t o = 0;
  L.bounds = o; o += al(sizeof(float) * 6 * P);
  L.grid = o; o += al(sizeof(StGrid) * P);
  L.pt_off = o; o += al(sizeof(int) * (P + 1));
  L.kr = o; o += al(sizeof(int) * 2 * P);
  L.occ = o; o += al((size_t)T);
  L.bur = o; o += al((size_t)T);
  L.blk = o; o += al(sizeof(int) * (nblk + 1));
  L.list = o; o += al(sizeof(int) * (size_t)T);
  L.parent = o; o += al(sizeof(int) * (size_t)T);
  L.cnt = o; o += al(sizeof(int) * (size_t)T);
  L.score = o; o += al(sizeof(int) * (size_t)T);
  L.sums = o; o += al(sizeof(unsigned long long) * 3 * (size_t)T);
  L.slot = o; o += al(sizeof(int) * (size_t)T);
  L.total = o;
  return L;
}

static int st_err(const std::string& s) {
  dbfr_set_error("dbfr_find_sites: " + s);
  return DBFR_ERR_ARG;
}

extern "C" int dbfr_sites_workspace_bytes(const dbfr_sites_in* in, size_t* bytes) {
  if (!in || !bytes) return st_err("null argument");
  if (in->n_prot < 0 || in->n_res < 0 || in->max_points < 0 || in->max_points > ST_MAX_POINTS)
    return st_err("n_prot / n_res negative or max_points outside [0, 2^30]");
  *bytes = st_layout(in->n_prot, in->max_points).total;
  return DBFR_OK;
}

extern "C" int dbfr_find_sites(const dbfr_sites_in* in, const dbfr_sites_opts* opts, const dbfr_sites_out* out, void* workspace,
                               size_t workspace_bytes, void* hip_stream) {
  if (!in || !out) return st_err("null argument");
  dbfr_sites_opts o = {1.0f, 1.2f, 8.0f, 4.0f, 6, 30, 5};
  if (opts) o = *opts;
  if (!(o.spacing >= 0.25f && o.spacing <= 4.f)) return st_err("spacing must lie in [0.25, 4] A");
  if (!(o.probe >= 0.f && o.probe <= 4.f)) return st_err("probe must lie in [0, 4] A");
  if (!(o.ray_length >= o.spacing && o.ray_length <= 255.f * o.spacing)) return st_err("ray_length must lie in [spacing, 255 spacing]");
  if (!(o.lining_cutoff >= 0.f && o.lining_cutoff <= 10.f)) return st_err("lining_cutoff must lie in [0, 10] A");
  if (o.min_buried < 1 || o.min_buried > 7) return st_err("min_buried must lie in [1, 7]");
  if (o.min_points < 1 || o.min_points > ST_MAX_PROT_POINTS) return st_err("min_points must lie in [1, 2^24]");
  if (o.max_sites < 1 || o.max_sites > ST_MAX_SITES) return st_err("max_sites must lie in [1, 64]");
  if (in->n_prot < 0 || in->n_res < 0 || in->max_points < 0 || in->max_points > ST_MAX_POINTS)
    return st_err("n_prot / n_res negative or max_points outside [0, 2^30]");
  if (in->n_prot == 0) return DBFR_OK;
  if (!in->res_ptr || (in->n_res > 0 && (!in->aatype || !in->atom37_pos || !in->atom37_mask || !in->radius)))
    return st_err("res_ptr / aatype / atom37_pos / atom37_mask / radius missing");
  if (!out->n_sites || !out->label || !out->n_points || !out->score || !out->centre) return st_err("n_sites / label / n_points / score / centre missing");
  const int P = in->n_prot;
  if (workspace_bytes < st_layout(P, 0).total || !workspace) return st_err("workspace too small");
  hipStream_t st = (hipStream_t)hip_stream;
  char* ws = (char*)workspace;
  StArgs a;
  a.in = *in;
  a.out = *out;
  a.h = o.spacing;
  a.probe = o.probe;
  a.cut = o.lining_cutoff;
  a.min_b = o.min_buried;
  a.min_pts = o.min_points;
  a.S = o.max_sites;
  a.tax = (int)std::floor((double)o.ray_length / (double)o.spacing);
  a.tdg = (int)std::floor((double)o.ray_length / ((double)o.spacing * std::sqrt(3.0)));
  StLayout L0 = st_layout(P, 0);
  a.bounds = (float*)(ws + L0.bounds);
  std::vector<int> rp(P + 1);
  HIPCHECK(hipMemcpyAsync(rp.data(), in->res_ptr, sizeof(int) * (P + 1), hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  if (rp[0] != 0 || rp[P] != in->n_res) return st_err("res_ptr must run from 0 to n_res");
  for (int p = 0; p < P; ++p)
    if (rp[p + 1] < rp[p]) return st_err("res_ptr must not decrease");
  // 1. the grid of every protein (read back: it sizes everything after)
  hipLaunchKernelGGL(k_sites_bounds, dim3((unsigned)P), dim3(ST_THREADS), 0, st, a);
  HIPCHECK(hipGetLastError());
  std::vector<float> bnd(6 * (size_t)P);
  HIPCHECK(hipMemcpyAsync(bnd.data(), a.bounds, sizeof(float) * bnd.size(), hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  std::vector<StGrid> grid(P);
  std::vector<int> pt_off(P + 1, 0);
  int64_t T = 0;
  for (int p = 0; p < P; ++p) {
    StGrid& G = grid[p];
    int64_t np = 1;
    for (int d = 0; d < 3; ++d) {
      const float mn = bnd[6 * p + d], mx = bnd[6 * p + 3 + d];
      if (!(mn <= mx)) { G.lo[d] = 0; G.n[d] = 0; np = 0; continue; }             // no atoms (or a NaN coordinate: refused below)
      const double l = std::floor((double)mn / (double)o.spacing), u = std::floor((double)mx / (double)o.spacing);
      if (!(u - l + 1 <= ST_MAX_AXIS) || !(std::fabs(l) < 1e9))
        return st_err("protein " + std::to_string(p) + ": grid over " + std::to_string(ST_MAX_AXIS) + " points along an axis");
      G.lo[d] = (int)l;
      G.n[d] = (int)(u - l) + 1;
      np *= G.n[d];
    }
    if (np == 0) for (int d = 0; d < 3; ++d) G.n[d] = 0;
    if (np > ST_MAX_PROT_POINTS) return st_err("protein " + std::to_string(p) + ": grid of " + std::to_string(np) + " points over 2^24");
    T += np;
    pt_off[p + 1] = (int)std::min<int64_t>(T, ST_MAX_POINTS);
    if (out->grid) for (int d = 0; d < 3; ++d) { out->grid[6 * p + d] = G.lo[d]; out->grid[6 * p + 3 + d] = G.n[d]; }
  }
  for (int p = 0; p < P; ++p)
    for (int d = 0; d < 3; ++d)
      if (std::isnan(bnd[6 * p + d]) || std::isnan(bnd[6 * p + 3 + d])) return st_err("protein " + std::to_string(p) + ": NaN coordinate");
  if (T > in->max_points) {
    dbfr_set_error("dbfr_find_sites: the grids hold " + std::to_string(T) + " points, over max_points = " + std::to_string(in->max_points));
    return DBFR_ERR_CAPACITY;
  }
  const StLayout L = st_layout(P, T);
  if (workspace_bytes < L.total) return st_err("workspace too small for the grids");
  a.total = (int)T;
  a.nblk = (int)((T + ST_THREADS - 1) / ST_THREADS);
  a.grid = (const StGrid*)(ws + L.grid);
  a.pt_off = (const int*)(ws + L.pt_off);
  a.kr = (int*)(ws + L.kr);
  a.occ = (uint8_t*)(ws + L.occ);
  a.bur = (uint8_t*)(ws + L.bur);
  a.blk = (int*)(ws + L.blk);
  a.list = (int*)(ws + L.list);
  a.parent = (int*)(ws + L.parent);
  a.cnt = (int*)(ws + L.cnt);
  a.score = (int*)(ws + L.score);
  a.sums = (unsigned long long*)(ws + L.sums);
  a.slot = (int*)(ws + L.slot);
  HIPCHECK(hipMemcpyAsync(ws + L.grid, grid.data(), sizeof(StGrid) * P, hipMemcpyHostToDevice, st));
  HIPCHECK(hipMemcpyAsync(ws + L.pt_off, pt_off.data(), sizeof(int) * (P + 1), hipMemcpyHostToDevice, st));
  HIPCHECK(hipStreamSynchronize(st));                  // (the host vectors die with this call)
  if (out->lining && in->n_res > 0) HIPCHECK(hipMemsetAsync(out->lining, 0, (size_t)in->n_res * o.max_sites, st));
  const unsigned blocks_atoms = (unsigned)(((int64_t)in->n_res * 37 + ST_THREADS - 1) / ST_THREADS);
  if (T > 0) {
    HIPCHECK(hipMemsetAsync(a.occ, 0, (size_t)T, st));
    if (out->labels) HIPCHECK(hipMemsetAsync(out->labels, 0xFF, sizeof(int) * (size_t)T, st));
    if (blocks_atoms) hipLaunchKernelGGL(k_sites_occ, dim3(blocks_atoms), dim3(ST_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_sites_burial, dim3((unsigned)a.nblk), dim3(ST_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_sites_scan, dim3(1), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(k_sites_compact, dim3((unsigned)a.nblk), dim3(ST_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_sites_union, dim3((unsigned)a.nblk), dim3(ST_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_sites_reduce, dim3((unsigned)a.nblk), dim3(ST_THREADS), 0, st, a);
    HIPCHECK(hipGetLastError());
  } else {
    HIPCHECK(hipMemsetAsync(a.blk, 0, sizeof(int), st));                         // nblk = 0: blk[0] = no pocket points
  }
  hipLaunchKernelGGL(k_sites_rank, dim3((unsigned)P), dim3(ST_THREADS), 0, st, a);
  if (out->lining && blocks_atoms) hipLaunchKernelGGL(k_sites_lining, dim3(blocks_atoms), dim3(ST_THREADS), 0, st, a);
  HIPCHECK(hipGetLastError());
  if (T > 0 && out->occupancy) HIPCHECK(hipMemcpyAsync(out->occupancy, a.occ, (size_t)T, hipMemcpyDeviceToDevice, st));
  if (T > 0 && out->burial) HIPCHECK(hipMemcpyAsync(out->burial, a.bur, (size_t)T, hipMemcpyDeviceToDevice, st));
  return DBFR_OK;
}
