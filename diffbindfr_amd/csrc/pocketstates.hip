// Pocket conformational states of the sampled poses: for every group (one complex) the chi angles and rotamer code of every
// (frame, residue), the rotamer statistics of every residue over the pose frames, and the all-pairs side-chain distance matrices of
// the frames with the per-residue mobility statistics.  include/dbfr.h states the definitions; docs/pocketstates.md the layout, the
// limits and the measurements.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/dbfr.h"
#include "common.h"
#include "frames.h"

#define RT_TABLE __device__ const
namespace ps_tables {
#include "residue_tables.inc"
}
#undef RT_TABLE

#define PS_THREADS FR_THREADS
#define PS_WAVES FR_WAVES
#define PS_TB 16                         // frames per tile: a tile pair holds at most 256 frame pairs, one per thread
#define PS_RC 8                          // residues per LDS chunk
#define PS_ROW 30                        // floats of the side-chain slots 4..13 of one residue
#define PS_STRIDE (PS_RC * PS_ROW + 1)   // floats per staged frame; odd, so the 16 column frames of a wave hit 16 different banks
#define PS_CODES 81                      // rotamer codes 0 .. 3^4 - 1
#define PS_SIDE 0x3FF0u                  // atom14 slots 4..13
#define PS_SQ_CLAMP 4096.f
#define PS_SQ_SCALE 1048576.f            // 2^20

struct PsArgs {
  dbfr_pocket_states_in in;
  dbfr_pocket_states_out out;
  int ref_all;                           // opts.ref_last, read where in.ref_last is NULL
  int tb;                                // frames per tile
};

__device__ __forceinline__ bool ps_has_ref(const PsArgs& a, int g) { return a.in.ref_last ? a.in.ref_last[g] != 0 : a.ref_all != 0; }
__device__ __forceinline__ bool ps_shape_ok(const PsArgs& a, int F, int R) { return F >= 0 && F <= a.in.max_frame && R >= 0 && R <= a.in.max_res; }
__device__ __forceinline__ bool ps_counted(const PsArgs& a, int row) { return !a.in.res_mask || a.in.res_mask[row] != 0; }

// ------------------------------------------------------------------------------------------------ every frame: chi, rot, frame_ok
// the dihedral p0-p1-p2-p3, IUPAC sign, the expression of apoholo.hip's ah_dihedral restated
__device__ __forceinline__ float ps_dihedral(const float* p0, const float* p1, const float* p2, const float* p3) {
  const float b1x = p1[0] - p0[0], b1y = p1[1] - p0[1], b1z = p1[2] - p0[2];
  const float b2x = p2[0] - p1[0], b2y = p2[1] - p1[1], b2z = p2[2] - p1[2];
  const float b3x = p3[0] - p2[0], b3y = p3[1] - p2[1], b3z = p3[2] - p2[2];
  const float n1x = b1y * b2z - b1z * b2y, n1y = b1z * b2x - b1x * b2z, n1z = b1x * b2y - b1y * b2x;
  const float n2x = b2y * b3z - b2z * b3y, n2y = b2z * b3x - b2x * b3z, n2z = b2x * b3y - b2y * b3x;
  const float l2 = sqrtf(b2x * b2x + b2y * b2y + b2z * b2z);
  const float y = l2 * (b1x * n2x + b1y * n2y + b1z * n2z), x = n1x * n2x + n1y * n2y + n1z * n2z;
  return atan2f(y, x);
}

// the bin of a defined chi (radians) as include/dbfr.h states it
__device__ __forceinline__ int ps_bin(float chi, bool pi_periodic) {
  float a = chi * 57.29577951308232f;
  if (pi_periodic) {
    if (a >= 135.f) a -= 180.f;
    if (a < -45.f) a += 180.f;
    return a < 45.f ? 0 : 1;
  }
  if (a < 0.f) a += 360.f;
  return a < 120.f ? 0 : (a < 240.f ? 1 : 2);
}

// One workgroup per frame: every thread checks present atoms of counted residues, then a thread per residue.
__global__ __launch_bounds__(PS_THREADS) void k_pocket_rot(PsArgs a) {
  const dbfr_pocket_states_in& in = a.in;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int g = frame_group(in.frame_ptr, in.n_group, f);
  const int k = f - in.frame_ptr[g], F = in.frame_ptr[g + 1] - in.frame_ptr[g];
  const int r0 = in.res_ptr[g], R = in.res_ptr[g + 1] - r0;
  const float nan = __builtin_nanf("");
  if (!ps_shape_ok(a, F, R)) {                                         // uniform over the workgroup; nothing of the frame is read
    if (R >= 0) {
      const long long row0 = in.pocket_off[g] + (long long)k * R;
      for (int s = tid; s < R; s += PS_THREADS) {
        for (int c = 0; c < 4; ++c) a.out.chi[4 * (row0 + s) + c] = nan;
        a.out.rot[row0 + s] = -1;
      }
    }
    if (tid == 0) a.out.frame_ok[f] = 0;
    return;
  }
  const long long row0 = in.pocket_off[g] + (long long)k * R;
  const float* x = in.pocket + 42 * row0;
  int bad = 0;
  for (int i = tid; i < 14 * R; i += PS_THREADS) {
    const int s = i / 14;
    if (ps_counted(a, r0 + s) && in.atom14_mask[14 * (size_t)r0 + i]) bad |= !atom_ok(x[3 * i], x[3 * i + 1], x[3 * i + 2]);
  }
  const bool unusable = __syncthreads_or(bad);
  if (tid == 0) a.out.frame_ok[f] = unusable ? 0 : 1;
  for (int s = tid; s < R; s += PS_THREADS) {
    const int aa = in.aatype[r0 + s];
    const bool known = aa >= 0 && aa < 20;
    const uint8_t* m = in.atom14_mask + 14 * (size_t)(r0 + s);
    const float* xr = x + 42 * (size_t)s;
    int code = 0, pw = 1;
    bool undefined = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float ang = nan;
      const bool defined = known && ps_tables::kChiMask[known ? aa : 20][c];
      if (defined && !unusable) {
        const int i0 = ps_tables::kChiAtoms14[aa][c][0], i1 = ps_tables::kChiAtoms14[aa][c][1], i2 = ps_tables::kChiAtoms14[aa][c][2],
                  i3 = ps_tables::kChiAtoms14[aa][c][3];
        if (m[i0] && m[i1] && m[i2] && m[i3]) ang = ps_dihedral(xr + 3 * i0, xr + 3 * i1, xr + 3 * i2, xr + 3 * i3);
      }
      if (defined) {
        if (ang == ang) code += pw * ps_bin(ang, ps_tables::kChiPiPeriodic[aa][c] != 0);
        else undefined = true;
      }
      pw *= 3;
      a.out.chi[4 * (row0 + s) + c] = ang;
    }
    a.out.rot[row0 + s] = (undefined || unusable) ? -1 : code;
  }
}

// ------------------------------------------------------------------------------------------------ every group: rotamer statistics
// One workgroup per group, a wave per residue: the lanes count the codes of the usable pose frames in an LDS histogram (integers),
// then read the number of codes seen, the most common one (ties: the smaller code) and the reference frame's.
__global__ __launch_bounds__(PS_THREADS) void k_pocket_rot_stats(PsArgs a) {
  __shared__ int hist[PS_WAVES][PS_CODES];
  __shared__ int used[PS_WAVES];
  const dbfr_pocket_states_in& in = a.in;
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f0 = in.frame_ptr[g], F = in.frame_ptr[g + 1] - f0;
  const int r0 = in.res_ptr[g], R = in.res_ptr[g + 1] - r0;
  if (!ps_shape_ok(a, F, R)) {
    for (int s = tid; s < R; s += PS_THREADS) {
      a.out.n_rot[r0 + s] = 0; a.out.top_rot[r0 + s] = -1; a.out.top_count[r0 + s] = 0;
      a.out.ref_rot[r0 + s] = -1; a.out.ref_count[r0 + s] = 0;
    }
    if (tid == 0) a.out.n_used[g] = 0;
    return;
  }
  const bool has_ref = ps_has_ref(a, g) && F >= 1;
  const int P = has_ref ? F - 1 : F;                                   // the pose frames
  int n = 0;
  for (int k = tid; k < P; k += PS_THREADS) n += a.out.frame_ok[f0 + k] != 0;
  n = wave_sum(n);
  if (lane == 0) used[wave] = n;
  __syncthreads();
  if (tid == 0) {
    int t = 0;
    for (int w = 0; w < PS_WAVES; ++w) t += used[w];
    a.out.n_used[g] = t;
  }
  const long long row0 = in.pocket_off[g];
  for (int s0 = 0; s0 < R; s0 += PS_WAVES) {                           // uniform over the workgroup
    const int s = s0 + wave;
    __syncthreads();                                                   // the histograms of the round before are read
    for (int c = lane; c < PS_CODES; c += 64) hist[wave][c] = 0;
    __syncthreads();
    const bool live = s < R && ps_counted(a, r0 + min(s, R - 1));
    if (live)
      for (int k = lane; k < P; k += 64) {
        const int code = a.out.rot[row0 + (long long)k * R + s];
        if (a.out.frame_ok[f0 + k] && code >= 0 && code < PS_CODES) atomicAdd(&hist[wave][code], 1);
      }
    __syncthreads();
    int seen = 0, key = 0;                                             // key = count * 128 + (127 - code): the maximum is the top code
    for (int c = lane; c < PS_CODES; c += 64) {
      const int cnt = hist[wave][c];
      seen += cnt > 0;
      if (cnt > 0) key = max(key, cnt * 128 + (127 - c));
    }
    seen = wave_sum(seen);
    for (int o = 32; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o));
    if (lane == 0 && s < R) {
      int rr = -1, rc = 0;
      if (live && has_ref) {
        rr = a.out.rot[row0 + (long long)(F - 1) * R + s];
        rc = rr >= 0 && rr < PS_CODES ? hist[wave][rr] : 0;
      }
      a.out.n_rot[r0 + s] = live ? seen : 0;
      a.out.top_rot[r0 + s] = live && key > 0 ? 127 - (key & 127) : -1;
      a.out.top_count[r0 + s] = live ? key >> 7 : 0;
      a.out.ref_rot[r0 + s] = rr;
      a.out.ref_count[r0 + s] = rc;
    }
  }
}

// ------------------------------------------------------------------------------------------------ every (pair tile, group): the matrices
// Grid (tile pair, group).  A group's frames are cut into tiles of TB <= 16 frames; the workgroup of tile pair (bi, bj), bi <= bj, owns
// the frame pairs i < j between them, ONE PER THREAD, and walks the residues in chunks of PS_RC: the side-chain slots of the chunk of
// both tiles' frames are staged in LDS, then every thread runs its pair's serial sums over the chunk's residues in ascending order.
// The sums of a pair never leave its thread, so they do not depend on the tiling; the per-residue statistics are maxima (a
// non-negative float's bits order as an unsigned integer) and integer sums: a wave reduction, LDS atomics across the waves, one
// global atomic per (workgroup, residue).
__global__ __launch_bounds__(PS_THREADS) void k_pocket_pairs(PsArgs a) {
  __shared__ float xs[2 * PS_TB * PS_STRIDE];
  __shared__ unsigned mob_bits[PS_RC], dev_bits[PS_RC];
  __shared__ unsigned long long mob_sq[PS_RC];
  __shared__ unsigned meta[PS_RC];                                     // bits 4..13: the side-chain slots; bit 16: counted; bit 17: q_sw is formed
  __shared__ int meta_aa[PS_RC];
  __shared__ unsigned char ok[2 * PS_TB];
  const dbfr_pocket_states_in& in = a.in;
  const dbfr_pocket_states_out& out = a.out;
  const int g = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int f0 = in.frame_ptr[g], F = in.frame_ptr[g + 1] - f0;
  const int r0 = in.res_ptr[g], R = in.res_ptr[g + 1] - r0;
  if (F <= 0) return;
  const float nan = __builtin_nanf("");
  const long long moff = in.pair_off[g];
  if (!ps_shape_ok(a, F, R)) {                                         // counts outside the stated maxima: NaN / -1, nothing else read
    if (blockIdx.x == 0)
      for (long long k = tid; k < (long long)F * F; k += PS_THREADS) {
        out.dist_max[moff + k] = nan; out.dist_pooled[moff + k] = nan; out.worst_res[moff + k] = -1;
      }
    return;
  }
  const int TB = a.tb, T = (F + TB - 1) / TB;
  if ((int)blockIdx.x >= T * (T + 1) / 2) return;                      // uniform over the workgroup
  int bi = 0, t = blockIdx.x;                                          // upper-triangle tile pair number t -> (bi, bj)
  while (t >= T - bi) { t -= T - bi; ++bi; }
  const int bj = bi + t;
  const int i0 = bi * TB, j0 = bj * TB, ni = min(TB, F - i0), nj = min(TB, F - j0);
  const bool diag = bi == bj;
  const int n_stage = diag ? ni : ni + nj;                             // staged frames: tile bi, then tile bj
  const int npairs = diag ? ni * (ni - 1) / 2 : ni * nj;
  int r = 0, c = 0;
  const bool live = tid < npairs;
  if (live) {
    if (diag) {                                                        // tid -> (r, c), r < c: row r holds ni - 1 - r pairs
      int kk = tid;
      while (kk >= ni - 1 - r) { kk -= ni - 1 - r; ++r; }
      c = r + 1 + kk;
    } else {
      r = tid / nj;
      c = tid - r * nj;
    }
  }
  const int fi = i0 + r, fj = j0 + c;
  if (tid < n_stage) ok[tid] = out.frame_ok[f0 + (tid < ni ? i0 + tid : j0 + tid - ni)];
  __syncthreads();
  const int cj = diag ? c : ni + c;                                    // the staged slot of frame fj
  const bool has_ref = ps_has_ref(a, g);
  const bool pair_ok = live && ok[r] && ok[cj];
  const bool pose_pair = pair_ok && !(has_ref && fj == F - 1);         // (fi < fj: only fj can be the last frame)
  const bool ref_pair = pair_ok && has_ref && fj == F - 1;
  const float* src = in.pocket + 42 * in.pocket_off[g];
  const float* xi = xs + r * PS_STRIDE;
  const float* xj = xs + cj * PS_STRIDE;
  float dmax = -1.f, qsum = 0.f;
  int worst = -1, nsum = 0;
  for (int s0 = 0; s0 < R; s0 += PS_RC) {
    const int nc = min(PS_RC, R - s0);
    __syncthreads();                                                   // the chunk before is read and flushed
    for (int idx = tid; idx < n_stage * PS_RC * PS_ROW; idx += PS_THREADS) {
      const int fl = idx / (PS_RC * PS_ROW), rem = idx - fl * (PS_RC * PS_ROW), sl = rem / PS_ROW, e = rem - sl * PS_ROW;
      if (sl < nc) {
        const int fr = fl < ni ? i0 + fl : j0 + fl - ni;
        xs[fl * PS_STRIDE + rem] = src[42 * ((size_t)fr * R + s0 + sl) + 12 + e];
      }
    }
    if (tid < PS_RC) {
      unsigned m = 0;
      int aa = 20;
      if (tid < nc) {
        const int row = r0 + s0 + tid;
        for (int at = 4; at < 14; ++at) m |= in.atom14_mask[14 * (size_t)row + at] ? 1u << at : 0u;
        const int t_aa = in.aatype[row];
        aa = t_aa >= 0 && t_aa < 20 ? t_aa : 20;
        bool swaps = false, closed = true;
        for (int at = 4; at < 14; ++at) {
          const int sw = ps_tables::kAtom14Swap[aa][at];
          swaps = swaps || sw != at;
          if ((m >> at) & 1u) closed = closed && ((m >> sw) & 1u);
        }
        if (ps_counted(a, row) && m) m |= 1u << 16;
        if (swaps && closed) m |= 1u << 17;
      }
      meta[tid] = m;
      meta_aa[tid] = aa;
      mob_bits[tid] = 0u;
      dev_bits[tid] = 0u;
      mob_sq[tid] = 0ull;
    }
    __syncthreads();
    for (int sl = 0; sl < nc; ++sl) {
      const unsigned m = meta[sl];
      if (!((m >> 16) & 1u)) continue;                                 // uniform over the workgroup
      const int n = __popc(m & PS_SIDE), aa = meta_aa[sl];
      float D = 0.f, msd = 0.f;
      if (pair_ok) {
        const float* pi = xi + sl * PS_ROW - 12;                       // slot `at` of the residue at pi + 3 at
        const float* pj = xj + sl * PS_ROW - 12;
        float q = 0.f;
#pragma unroll
        for (int at = 4; at < 14; ++at)
          if ((m >> at) & 1u) {
            const float dx = pi[3 * at] - pj[3 * at], dy = pi[3 * at + 1] - pj[3 * at + 1], dz = pi[3 * at + 2] - pj[3 * at + 2];
            q += dx * dx + dy * dy + dz * dz;
          }
        if ((m >> 17) & 1u) {
          float qs = 0.f;
#pragma unroll
          for (int at = 4; at < 14; ++at)
            if ((m >> at) & 1u) {
              const int sw = ps_tables::kAtom14Swap[aa][at];
              const float dx = pi[3 * at] - pj[3 * sw], dy = pi[3 * at + 1] - pj[3 * sw + 1], dz = pi[3 * at + 2] - pj[3 * sw + 2];
              qs += dx * dx + dy * dy + dz * dz;
            }
          q = fminf(q, qs);
        }
        msd = q / (float)n;
        D = sqrtf(msd);
        qsum += q;
        nsum += n;
        if (D > dmax) { dmax = D; worst = s0 + sl; }
      }
      // the residue's statistics over the workgroup's pairs: maxima and an integer sum
      float vm = pose_pair ? D : 0.f, vd = ref_pair ? D : 0.f;
      long long sq = pose_pair ? llrintf(fminf(msd, PS_SQ_CLAMP) * PS_SQ_SCALE) : 0ll;
      vm = wave_max(vm);
      vd = wave_max(vd);
      for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
      if (lane == 0) {
        if (vm > 0.f) atomicMax(&mob_bits[sl], __float_as_uint(vm));
        if (vd > 0.f) atomicMax(&dev_bits[sl], __float_as_uint(vd));
        if (sq) atomicAdd(&mob_sq[sl], (unsigned long long)sq);
      }
    }
    __syncthreads();
    if (tid < nc) {
      const size_t row = (size_t)r0 + s0 + tid;
      if (mob_bits[tid]) atomicMax(reinterpret_cast<unsigned*>(out.mob_max) + row, mob_bits[tid]);
      if (dev_bits[tid]) atomicMax(reinterpret_cast<unsigned*>(out.dev_ref_max) + row, dev_bits[tid]);
      if (mob_sq[tid]) atomicAdd(reinterpret_cast<unsigned long long*>(out.mob_sq) + row, mob_sq[tid]);
    }
  }
  if (live) {
    const float vmax = pair_ok ? (worst >= 0 ? dmax : 0.f) : nan;
    const float vpool = pair_ok ? (nsum > 0 ? sqrtf(qsum / (float)nsum) : 0.f) : nan;
    const int w = pair_ok ? worst : -1;
    const long long ij = moff + (long long)fi * F + fj, ji = moff + (long long)fj * F + fi;
    out.dist_max[ij] = vmax; out.dist_max[ji] = vmax;
    out.dist_pooled[ij] = vpool; out.dist_pooled[ji] = vpool;
    out.worst_res[ij] = w; out.worst_res[ji] = w;
  }
  if (diag && tid < ni) {
    const long long dd = moff + (long long)(i0 + tid) * F + i0 + tid;
    const float v = ok[tid] ? 0.f : nan;
    out.dist_max[dd] = v; out.dist_pooled[dd] = v; out.worst_res[dd] = -1;
  }
}

// ------------------------------------------------------------------------------------------------ host
static int ps_validate(const dbfr_pocket_states_in& d, const dbfr_pocket_states_in& h, int ref_all) {
  const char* fn = "dbfr_pocket_states";
  if (!h.frame_ptr || !h.res_ptr || !h.pocket_off || !h.pair_off || (d.ref_last && !h.ref_last))
    return arg_err(fn, "host: a host copy of frame_ptr / res_ptr / pocket_off / pair_off / ref_last is missing");
  const int G = d.n_group;
  if (const int rc = frame_ptr_err(fn, h.frame_ptr, G, d.n_frame)) return rc;
  if (h.res_ptr[0] != 0) return arg_err(fn, "res_ptr does not start at 0");
  long long rows = 0, cells = 0;
  for (int g = 0; g < G; ++g) {
    const std::string where = "group " + std::to_string(g) + ": ";
    const long long F = (long long)h.frame_ptr[g + 1] - h.frame_ptr[g], R = (long long)h.res_ptr[g + 1] - h.res_ptr[g];
    if (const int rc = group_counts_err(fn, where, {{F, "frames", "max_frame", d.max_frame}, {R, "pocket rows", "max_res", d.max_res}})) return rc;
    if (h.pocket_off[g] != rows || h.pair_off[g] != cells)
      return arg_err(fn, where + "pocket_off / pair_off is not the running sum of the groups before it");
    rows += F * R;
    cells += F * F;
    const bool ref = d.ref_last ? h.ref_last[g] != 0 : ref_all != 0;
    if (ref && F == 1) return arg_err(fn, where + "a reference frame and no pose frame (ref_last with one frame)");
  }
  return DBFR_OK;
}

extern "C" int dbfr_pocket_states(const dbfr_pocket_states_in* in, const dbfr_pocket_states_opts* opts, const dbfr_pocket_states_out* out,
                                  void* hip_stream) {
  const char* fn = "dbfr_pocket_states";
  if (!in || !out) return arg_err(fn, "null argument");
  if (in->n_group < 0 || in->n_frame < 0) return arg_err(fn, "negative n_group / n_frame");
  if (in->n_group > 65535) return arg_err(fn, "more than 65535 groups in one launch");
  if (in->max_frame < 0 || in->max_frame > DBFR_PKS_MAX_FRAME) return limit_err(fn, "max_frame (frames of a group)", in->max_frame, 0, DBFR_PKS_MAX_FRAME);
  if (in->max_res < 0 || in->max_res > DBFR_PKS_MAX_RES) return limit_err(fn, "max_res (pocket rows)", in->max_res, 0, DBFR_PKS_MAX_RES);
  dbfr_pocket_states_opts o = {0, 0};
  if (opts) o = *opts;
  if (o.ref_last != 0 && o.ref_last != 1) return arg_err(fn, "ref_last must be 0 or 1");
  if (o.tile_rows < 0) return arg_err(fn, "negative tile_rows");
  if (in->n_group == 0) return in->n_frame == 0 ? DBFR_OK : arg_err(fn, "frames without groups");
  if (!in->frame_ptr || !in->res_ptr || !in->pocket_off || !in->pocket || !in->aatype || !in->atom14_mask || !in->pair_off)
    return arg_err(fn, "frame_ptr / res_ptr / pocket_off / pocket / aatype / atom14_mask / pair_off missing");
  if (!out->dist_max || !out->dist_pooled || !out->worst_res || !out->chi || !out->rot || !out->n_rot || !out->top_rot || !out->top_count ||
      !out->ref_rot || !out->ref_count || !out->mob_max || !out->mob_sq || !out->dev_ref_max || !out->n_used || !out->frame_ok)
    return arg_err(fn, "an output array is missing");
  if (!in->host) return arg_err(fn, "in.host (the host copies of the index arrays) is missing: the counts are validated before every launch");
  const dbfr_pocket_states_in& h = *static_cast<const dbfr_pocket_states_in*>(in->host);
  if (const int rc = ps_validate(*in, h, o.ref_last)) return rc;
  PsArgs a;
  a.in = *in;
  a.in.host = nullptr;
  a.out = *out;
  a.ref_all = o.ref_last;
  a.tb = o.tile_rows > 0 ? std::min(PS_TB, o.tile_rows) : PS_TB;
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t n_res = (size_t)h.res_ptr[in->n_group];
  if (n_res) {
    HIPCHECK(hipMemsetAsync(out->mob_max, 0, sizeof(float) * n_res, st));
    HIPCHECK(hipMemsetAsync(out->mob_sq, 0, sizeof(int64_t) * n_res, st));
    HIPCHECK(hipMemsetAsync(out->dev_ref_max, 0, sizeof(float) * n_res, st));
  }
  if (in->n_frame > 0) HIPCHECK(launch_frames(k_pocket_rot, in->n_frame, PS_THREADS, 0, st, a));
  hipLaunchKernelGGL(k_pocket_rot_stats, dim3((unsigned)in->n_group), dim3(PS_THREADS), 0, st, a);
  HIPCHECK(hipGetLastError());
  if (in->n_frame == 0 || in->max_frame == 0) return DBFR_OK;
  const int T = (in->max_frame + a.tb - 1) / a.tb;
  hipLaunchKernelGGL(k_pocket_pairs, dim3((unsigned)(T * (T + 1) / 2), (unsigned)in->n_group), dim3(PS_THREADS), 0, st, a);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}
