// In-place Gaussian shape and feature overlap of conformations: for every cloud (one molecule in one conformation) its self overlap,
// and for every set the block A x B of pair overlaps, per point kind, as integer sums of float32 pair terms -- with the Tanimoto
// read-outs and the distance that dbfr_select_modes clusters on.  include/dbfr.h states the definitions; docs/shapesim.md the layout,
// the limits and the measurements.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/dbfr.h"
#include "common.h"
#include "frames.h"

#define SH_THREADS FR_THREADS
#define SH_WAVES FR_WAVES
#define SH_KINDS DBFR_SHAPE_KINDS
#define SH_BTILE 32                                  // clouds of B per workgroup where opts.b_tile is 0
#define SH_LDS_POINTS (4 * DBFR_SHAPE_MAX_ATOMS + DBFR_SHAPE_MAX_GROUPS)   // what 256 atoms and 32 groups can expand to; a usable cloud has <= 1024
#define SH_PI_F 3.14159274f
#define SH_ALPHA_MIN 0.1f
#define SH_ALPHA_MAX 1e4f

struct ShArgs {
  dbfr_shape_in in;
  dbfr_shape_out out;
  double w;                                          // (double)opts.color_weight
  int b_tile;
};

// the molecule of a cloud as the kernels read it
struct ShCloud {
  const float* x;                                    // [N, 3] this conformation
  const float* alpha;
  const uint8_t* flags;
  const int32_t* grp;                                // [LG, 8]
  float color_alpha;
  int N, LG;
  bool shape_ok;                                     // the device-side counts are within the limits (else nothing of the cloud is read)
};

__device__ __forceinline__ ShCloud sh_cloud(const dbfr_shape_in& in, int c) {
  ShCloud k;
  const int m = in.cloud_mol[c];
  const int a0 = in.mol_atom_ptr[m], g0 = in.mol_grp_ptr[m];
  k.N = in.mol_atom_ptr[m + 1] - a0;
  k.LG = in.mol_grp_ptr[m + 1] - g0;
  k.x = in.pos + 3 * in.cloud_pos_off[c];
  k.alpha = in.alpha + a0;
  k.flags = in.flags + a0;
  k.grp = in.grp + 8 * (size_t)g0;
  k.color_alpha = in.color_alpha[m];
  k.shape_ok = k.N >= 1 && k.N <= DBFR_SHAPE_MAX_ATOMS && k.LG >= 0 && k.LG <= DBFR_SHAPE_MAX_GROUPS;
  return k;
}

// the point kind of a group kind (0 ring / 1 cation / 2 anion -> 5 / 3 / 4)
__device__ __forceinline__ int sh_group_kind(int gk) { return gk == 0 ? 5 : (gk == 1 ? 3 : 4); }

// the centroid of a group in this conformation: one serial float32 sum in list order, divided by the count
__device__ __forceinline__ void sh_centroid(const ShCloud& k, const int32_t* row, float& cx, float& cy, float& cz) {
  float sx = 0.f, sy = 0.f, sz = 0.f;
  int n = 0;
#pragma unroll
  for (int q = 1; q <= 6; ++q) {
    const int i = row[q];
    if (i >= 0 && i < k.N) {
      sx += k.x[3 * i]; sy += k.x[3 * i + 1]; sz += k.x[3 * i + 2];
      ++n;
    }
  }
  const float d = (float)max(n, 1);
  cx = sx / d; cy = sy / d; cz = sz / d;
}

// The pair term of include/dbfr.h in two steps.  What depends on the two widths alone: q = (aa ab) / (aa + ab) and the prefactor
// (8 c) sqrtf(c), c = PI_F / (aa + ab) -- aa + ab and aa * ab commute, so the two points may be swapped ...
struct ShWidths {
  float q, pref;
};
__device__ __forceinline__ ShWidths sh_widths(float aa, float ab) {
  const float s = aa + ab;
  const float c = SH_PI_F / s;
  return {(aa * ab) / s, (8.0f * c) * sqrtf(c)};
}
// ... and the term itself: swapping the points negates dx, dy, dz exactly.  The same bits either way round.
__device__ __forceinline__ long long sh_term(const ShWidths& w, float xa, float ya, float za, float xb, float yb, float zb) {
  const float dx = xa - xb, dy = ya - yb, dz = za - zb;
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  const float v = w.pref * expf(-(w.q * d2));
  return llrint((double)v * 4294967296.0);
}

// the integer sum of the terms of one point against the staged points [first, last): every lane reads the same LDS address.  The
// staged points of a kind are sorted by width (sh_stage), so the two divisions and the square root of sh_widths run once per
// distinct width of the range, not once per point: the values are the ones the unhoisted expression gives.
__device__ __forceinline__ long long sh_walk(const float4* pts, int first, int last, float x, float y, float z, float al) {
  long long acc = 0;
  float width = -1.f;                                                  // (no staged width is negative)
  ShWidths w = {0.f, 0.f};
  for (int i = first; i < last; ++i) {
    const float4 p = pts[i];
    if (p.w != width) {                                                // uniform over the wave: p is a broadcast read
      width = p.w;
      w = sh_widths(p.w, al);
    }
    acc += sh_term(w, p.x, p.y, p.z, x, y, z);
  }
  return acc;
}

// Cloud `k` expanded into LDS by the whole workgroup, sorted by kind: pts[kf[q] .. kf[q + 1]) are the points of kind q, the shape
// points sorted by width (the others share one).  Thread t owns atom t; donors, acceptors and hydrophobes are compacted in atom
// order, thread j owns group j.  Returns true (uniform) when the cloud is unusable: a coordinate fails atom_ok, or the counts are
// outside the limits.
__device__ __forceinline__ bool sh_stage(const ShCloud& k, float4* pts, int* kf, int* wcnt, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  if (!k.shape_ok) return true;
  const bool mine = tid < k.N;
  float x = 0.f, y = 0.f, z = 0.f, al = 0.f;
  int fl = 0;
  if (mine) {
    x = k.x[3 * tid]; y = k.x[3 * tid + 1]; z = k.x[3 * tid + 2];
    fl = k.flags[tid];
    al = k.alpha[tid];
    pts[tid].w = al;
  }
  int bad = mine && !atom_ok(x, y, z);
  int n_cat = 0, n_an = 0, n_ring = 0, before = 0, gk = 0;
  if (tid < k.LG) gk = k.grp[8 * tid];
  for (int j = 0; j < k.LG; ++j) {                                     // uniform: at most 32 kinds, the same address in every lane
    const int kj = k.grp[8 * j];
    n_ring += kj == 0; n_cat += kj == 1; n_an += kj == 2;
    before += j < tid && kj == gk;
  }
  bad |= n_ring + n_cat + n_an != k.LG;                                // a kind outside 0..2
  bad = __syncthreads_or(bad);
  int rank = 0;                                                        // the atom's place among the shape points, by width, then by index
  for (int j = 0; j < k.N; ++j) {
    const float aj = pts[j].w;
    rank += aj < al || (aj == al && j < tid);
  }
  __syncthreads();                                                     // every width is read
  if (mine) pts[rank] = make_float4(x, y, z, al);
  const float4 cp = make_float4(x, y, z, k.color_alpha);
  int slot, n_don, n_acc, n_hyd;
  block_compact(mine && (fl & 1), k.N, wcnt, lane, wave, slot, n_don);
  if (mine && (fl & 1)) pts[slot] = cp;
  __syncthreads();
  const int b2 = k.N + n_don;
  block_compact(mine && (fl & 2), b2, wcnt, lane, wave, slot, n_acc);
  if (mine && (fl & 2)) pts[slot] = cp;
  __syncthreads();
  const int b3 = b2 + n_acc, b4 = b3 + n_cat, b5 = b4 + n_an, b6 = b5 + n_ring;
  block_compact(mine && (fl & 4), b6, wcnt, lane, wave, slot, n_hyd);
  if (mine && (fl & 4)) pts[slot] = cp;
  if (tid < k.LG && !bad) {
    float cx, cy, cz;
    sh_centroid(k, k.grp + 8 * tid, cx, cy, cz);
    pts[(gk == 0 ? b5 : (gk == 1 ? b3 : b4)) + before] = make_float4(cx, cy, cz, k.color_alpha);
  }
  if (tid == 0) {
    kf[0] = 0; kf[1] = k.N; kf[2] = b2; kf[3] = b3; kf[4] = b4; kf[5] = b5; kf[6] = b6; kf[7] = b6 + n_hyd;
  }
  __syncthreads();
  return bad || b6 + n_hyd > DBFR_SHAPE_MAX_POINTS;
}

// The points of cloud `k` owned by thread t of S against the staged cloud: acc[q] += the thread's share of O[., ., q].  The points
// of `k` need no order (the sums are integer sums): an atom gives its shape point and a point per flag bit, a group its centroid.
// Returns true when a coordinate the thread read fails atom_ok (or the cloud's counts are outside the limits).
__device__ __forceinline__ bool sh_against(const ShCloud& k, const float4* pts, const int* kf, int t, int S, long long (&acc)[SH_KINDS]) {
  if (!k.shape_ok) return true;
  bool bad = false;
  for (int i = t; i < k.N; i += S) {
    const float x = k.x[3 * i], y = k.x[3 * i + 1], z = k.x[3 * i + 2];
    const int fl = k.flags[i];
    bad = bad || !atom_ok(x, y, z);
    acc[0] += sh_walk(pts, kf[0], kf[1], x, y, z, k.alpha[i]);
    if (fl & 1) acc[1] += sh_walk(pts, kf[1], kf[2], x, y, z, k.color_alpha);
    if (fl & 2) acc[2] += sh_walk(pts, kf[2], kf[3], x, y, z, k.color_alpha);
    if (fl & 4) acc[6] += sh_walk(pts, kf[6], kf[7], x, y, z, k.color_alpha);
  }
  for (int j = t; j < k.LG; j += S) {
    const int gk = k.grp[8 * j];
    if (gk < 0 || gk > 2) { bad = true; continue; }
    float cx, cy, cz;
    sh_centroid(k, k.grp + 8 * j, cx, cy, cz);
    const int pk = sh_group_kind(gk);
    const long long v = sh_walk(pts, kf[pk], kf[pk + 1], cx, cy, cz, k.color_alpha);
    acc[3] += pk == 3 ? v : 0ll;
    acc[4] += pk == 4 ? v : 0ll;
    acc[5] += pk == 5 ? v : 0ll;
  }
  return bad;
}

__device__ __forceinline__ long long sh_wave_sum(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ------------------------------------------------------------------------------------------------ every cloud: self_fixed
// One workgroup per cloud: the cloud staged in LDS, then its own points, one atom (and one group) per thread, against it.
__global__ __launch_bounds__(SH_THREADS) void k_shape_self(ShArgs a) {
  __shared__ float4 pts[SH_LDS_POINTS];
  __shared__ int kf[8];
  __shared__ int wcnt[SH_WAVES];
  __shared__ long long red[SH_WAVES][SH_KINDS];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ShCloud k = sh_cloud(a.in, c);
  const bool bad = sh_stage(k, pts, kf, wcnt, tid);                    // uniform
  long long acc[SH_KINDS] = {0, 0, 0, 0, 0, 0, 0};
  if (!bad) sh_against(k, pts, kf, tid, SH_THREADS, acc);
#pragma unroll
  for (int q = 0; q < SH_KINDS; ++q) {
    const long long v = sh_wave_sum(acc[q]);
    if (lane == 0) red[wave][q] = v;
  }
  __syncthreads();
  if (tid < SH_KINDS) {
    long long v = 0;
    for (int w = 0; w < SH_WAVES; ++w) v += red[w][tid];
    a.out.self_fixed[(size_t)SH_KINDS * c + tid] = bad ? INT64_MIN : v;
  }
}

// ------------------------------------------------------------------------------------------------ every (tile of B, cloud of A, set)
// Grid (tile of B, index in A, set).  Cloud a is staged once in LDS; every wave takes the tile's clouds of B in turn with its lanes
// over b's atoms and groups, each lane walking only a's range of the kind of its point.  One int64 accumulator per kind and lane,
// integer wave sums, then lane 0 stores the row and its read-outs.
__global__ __launch_bounds__(SH_THREADS) void k_shape_pairs(ShArgs a) {
  __shared__ float4 pts[SH_LDS_POINTS];
  __shared__ int kf[8];
  __shared__ int wcnt[SH_WAVES];
  const dbfr_shape_in& in = a.in;
  const int s = blockIdx.z, ia = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool same = in.b_ptr == nullptr;
  const int a0 = in.a_ptr[s], nA = in.a_ptr[s + 1] - a0;
  const int b0 = same ? a0 : in.b_ptr[s], nB = same ? nA : in.b_ptr[s + 1] - b0;
  const int32_t* bcl = same ? in.a_cloud : in.b_cloud;
  const int j0 = (int)blockIdx.x * a.b_tile;
  if (ia >= nA || j0 >= nB) return;                                    // uniform over the workgroup
  const int j1 = min(nB, j0 + a.b_tile);
  const int ca = in.a_cloud[a0 + ia];
  const bool a_bad = sh_stage(sh_cloud(in, ca), pts, kf, wcnt, tid);   // uniform
  const double nan = __builtin_nan("");
  for (int j = j0 + wave; j < j1; j += SH_WAVES) {                     // uniform over the wave
    const int cb = bcl[b0 + j];
    long long acc[SH_KINDS] = {0, 0, 0, 0, 0, 0, 0};
    bool bad = a_bad;
    if (!a_bad) bad = sh_against(sh_cloud(in, cb), pts, kf, lane, 64, acc);
    bad = __any(bad) != 0;
#pragma unroll
    for (int q = 0; q < SH_KINDS; ++q) acc[q] = sh_wave_sum(acc[q]);
    if (lane != 0) continue;
    const long long row = in.pair_off[s] + (long long)ia * nB + j;
    if (a.out.pair_fixed) {
#pragma unroll
      for (int q = 0; q < SH_KINDS; ++q) a.out.pair_fixed[SH_KINDS * row + q] = bad ? INT64_MIN : acc[q];
    }
    if (!a.out.tanimoto && !a.out.dist) continue;
    const int64_t* sa = a.out.self_fixed + (size_t)SH_KINDS * ca;
    const int64_t* sb = a.out.self_fixed + (size_t)SH_KINDS * cb;
    bad = bad || sa[0] == INT64_MIN || sb[0] == INT64_MIN;
    double ts = nan, tc = nan, d = nan;
    if (!bad) {
      long long c_ab = 0, c_aa = 0, c_bb = 0;
#pragma unroll
      for (int q = 1; q < SH_KINDS; ++q) { c_ab += acc[q]; c_aa += sa[q]; c_bb += sb[q]; }
      ts = (double)acc[0] / (((double)sa[0] + (double)sb[0]) - (double)acc[0]);
      if (c_aa + c_bb != 0) tc = (double)c_ab / (((double)c_aa + (double)c_bb) - (double)c_ab);
      const double sim = (c_aa == 0 || c_bb == 0) ? ts : ((1.0 - a.w) * ts) + (a.w * tc);
      d = (same && ia == j) ? 0.0 : 1.0 - sim;
    }
    if (a.out.tanimoto) { a.out.tanimoto[2 * row] = (float)ts; a.out.tanimoto[2 * row + 1] = (float)tc; }
    if (a.out.dist) a.out.dist[row] = (float)d;
  }
}

// ------------------------------------------------------------------------------------------------ host
static int sh_validate(const dbfr_shape_in& d, const dbfr_shape_in& h) {
  const char* fn = "dbfr_shape_overlap";
  if (!h.mol_atom_ptr || !h.alpha || !h.flags || !h.color_alpha || !h.mol_grp_ptr || !h.grp || !h.cloud_mol || !h.cloud_pos_off || !h.a_ptr ||
      !h.a_cloud || !h.pair_off || (d.b_ptr && (!h.b_ptr || !h.b_cloud)))
    return arg_err(fn, "host: a host copy of an index array is missing (every array but pos)");
  if (h.mol_atom_ptr[0] != 0 || h.mol_grp_ptr[0] != 0) return arg_err(fn, "mol_atom_ptr / mol_grp_ptr does not start at 0");
  for (int m = 0; m < d.n_mol; ++m) {
    const std::string where = "molecule " + std::to_string(m) + ": ";
    const long long N = (long long)h.mol_atom_ptr[m + 1] - h.mol_atom_ptr[m], LG = (long long)h.mol_grp_ptr[m + 1] - h.mol_grp_ptr[m];
    if (N < 1 || N > DBFR_SHAPE_MAX_ATOMS) return arg_err(fn, where + std::to_string(N) + " atoms outside [1, " + std::to_string(DBFR_SHAPE_MAX_ATOMS) + "]");
    if (LG < 0 || LG > DBFR_SHAPE_MAX_GROUPS)
      return arg_err(fn, where + std::to_string(LG) + " groups outside [0, " + std::to_string(DBFR_SHAPE_MAX_GROUPS) + "]");
    const float ca = h.color_alpha[m];
    if (!(ca >= SH_ALPHA_MIN && ca <= SH_ALPHA_MAX)) return arg_err(fn, where + "color_alpha lies outside [0.1, 1e4]");
    long long points = N + LG;
    for (long long i = h.mol_atom_ptr[m]; i < h.mol_atom_ptr[m + 1]; ++i) {
      if (!(h.alpha[i] >= SH_ALPHA_MIN && h.alpha[i] <= SH_ALPHA_MAX))
        return arg_err(fn, where + "the alpha of atom " + std::to_string(i - h.mol_atom_ptr[m]) + " lies outside [0.1, 1e4]");
      if (h.flags[i] > 7) return arg_err(fn, where + "the flags of atom " + std::to_string(i - h.mol_atom_ptr[m]) + " set a bit beyond 0..2");
      points += __builtin_popcount(h.flags[i]);
    }
    if (points > DBFR_SHAPE_MAX_POINTS)
      return arg_err(fn, where + std::to_string(points) + " points, at most " + std::to_string(DBFR_SHAPE_MAX_POINTS) + " per cloud");
    for (long long j = h.mol_grp_ptr[m]; j < h.mol_grp_ptr[m + 1]; ++j) {
      const int32_t* row = h.grp + 8 * j;
      if (row[0] < 0 || row[0] > 2 || row[1] < 0) return arg_err(fn, where + "a group needs a kind in 0..2 and at least one atom");
      for (int q = 1; q <= 6; ++q)
        if (row[q] < -1 || row[q] >= N) return arg_err(fn, where + "a group atom index lies outside its " + std::to_string(N) + " atoms");
    }
  }
  for (int c = 0; c < d.n_cloud; ++c) {
    const int m = h.cloud_mol[c];
    if (m < 0 || m >= d.n_mol) return arg_err(fn, "cloud " + std::to_string(c) + ": its molecule " + std::to_string(m) + " is out of range");
    const long long N = (long long)h.mol_atom_ptr[m + 1] - h.mol_atom_ptr[m];
    if (h.cloud_pos_off[c] < 0 || h.cloud_pos_off[c] + N > d.n_pos_row)
      return arg_err(fn, "cloud " + std::to_string(c) + ": its position rows lie outside pos (" + std::to_string(d.n_pos_row) + " rows)");
  }
  if (h.a_ptr[0] != 0 || (d.b_ptr && h.b_ptr[0] != 0)) return arg_err(fn, "a_ptr / b_ptr does not start at 0");
  long long rows = 0;
  for (int s = 0; s < d.n_set; ++s) {
    const std::string where = "set " + std::to_string(s) + ": ";
    const long long nA = (long long)h.a_ptr[s + 1] - h.a_ptr[s], nB = d.b_ptr ? (long long)h.b_ptr[s + 1] - h.b_ptr[s] : nA;
    if (const int rc = group_counts_err(fn, where, {{nA, "clouds in A", "max_a", d.max_a}, {nB, "clouds in B", "max_b", d.b_ptr ? d.max_b : d.max_a}}))
      return rc;
    if (h.pair_off[s] != rows) return arg_err(fn, where + "pair_off is not the running sum of the sets before it");
    rows += nA * nB;
    for (long long i = h.a_ptr[s]; i < h.a_ptr[s + 1]; ++i)
      if (h.a_cloud[i] < 0 || h.a_cloud[i] >= d.n_cloud) return arg_err(fn, where + "a cloud index of A is out of range");
    if (d.b_ptr)
      for (long long i = h.b_ptr[s]; i < h.b_ptr[s + 1]; ++i)
        if (h.b_cloud[i] < 0 || h.b_cloud[i] >= d.n_cloud) return arg_err(fn, where + "a cloud index of B is out of range");
  }
  return DBFR_OK;
}

extern "C" int dbfr_shape_overlap(const dbfr_shape_in* in, const dbfr_shape_opts* opts, const dbfr_shape_out* out, void* hip_stream) {
  const char* fn = "dbfr_shape_overlap";
  if (!in || !out) return arg_err(fn, "null argument");
  if (in->n_mol < 0 || in->n_cloud < 0 || in->n_set < 0 || in->n_pos_row < 0) return arg_err(fn, "negative n_mol / n_cloud / n_set / n_pos_row");
  if (in->n_set > 65535) return arg_err(fn, "more than 65535 sets in one launch");
  if (in->max_a < 0 || in->max_a > DBFR_SHAPE_MAX_SIDE) return limit_err(fn, "max_a (clouds in A)", in->max_a, 0, DBFR_SHAPE_MAX_SIDE);
  if (in->max_b < 0 || in->max_b > DBFR_SHAPE_MAX_SIDE) return limit_err(fn, "max_b (clouds in B)", in->max_b, 0, DBFR_SHAPE_MAX_SIDE);
  dbfr_shape_opts o = {0.5f, 0};
  if (opts) o = *opts;
  if (!(o.color_weight >= 0.f && o.color_weight <= 1.f)) return arg_err(fn, "color_weight must lie in [0, 1] and must not be NaN");
  if (o.b_tile < 0) return arg_err(fn, "negative b_tile");
  if ((out->tanimoto || out->dist) && !out->self_fixed) return arg_err(fn, "tanimoto / dist read self_fixed, which is missing");
  if (in->n_cloud == 0) return in->n_set == 0 || in->max_a == 0 ? DBFR_OK : arg_err(fn, "sets without clouds");
  if (in->n_mol == 0) return arg_err(fn, "clouds without molecules");
  if (!in->mol_atom_ptr || !in->alpha || !in->flags || !in->color_alpha || !in->mol_grp_ptr || !in->grp || !in->cloud_mol || !in->cloud_pos_off ||
      !in->pos)
    return arg_err(fn, "mol_atom_ptr / alpha / flags / color_alpha / mol_grp_ptr / grp / cloud_mol / cloud_pos_off / pos missing");
  if (in->n_set > 0 && (!in->a_ptr || !in->a_cloud || !in->pair_off || (in->b_ptr && !in->b_cloud)))
    return arg_err(fn, "a_ptr / a_cloud / pair_off (or b_cloud under b_ptr) missing");
  if (!in->host) return arg_err(fn, "in.host (the host copies of the index arrays) is missing: the counts are validated before every launch");
  const dbfr_shape_in& h = *static_cast<const dbfr_shape_in*>(in->host);
  if (const int rc = sh_validate(*in, h)) return rc;
  ShArgs a;
  a.in = *in;
  a.in.host = nullptr;
  a.out = *out;
  a.w = (double)o.color_weight;
  a.b_tile = o.b_tile > 0 ? std::min(o.b_tile, DBFR_SHAPE_MAX_SIDE) : SH_BTILE;
  hipStream_t st = (hipStream_t)hip_stream;
  if (out->self_fixed) {
    hipLaunchKernelGGL(k_shape_self, dim3((unsigned)in->n_cloud), dim3(SH_THREADS), 0, st, a);
    HIPCHECK(hipGetLastError());
  }
  const int max_b = in->b_ptr ? in->max_b : in->max_a;
  if (in->n_set == 0 || in->max_a == 0 || max_b == 0 || (!out->pair_fixed && !out->tanimoto && !out->dist)) return DBFR_OK;
  hipLaunchKernelGGL(k_shape_pairs, dim3((unsigned)((max_b + a.b_tile - 1) / a.b_tile), (unsigned)in->max_a, (unsigned)in->n_set), dim3(SH_THREADS),
                     0, st, a);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}
