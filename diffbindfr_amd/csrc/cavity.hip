// Cavity volume and ligand fill of each pose's pocket: the LIGSITE-style definition of docs/sites.md (occupancy, burial along 7
// lines, 6-connected components) evaluated per frame on a 32^3 lattice that lives in LDS as bit planes, for every frame of a ragged
// batch, in one launch.  include/dbfr.h states the outputs; docs/cavity.md the specification, the layout and the limits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/dbfr.h"
#include "common.h"
#include "frames.h"

// One workgroup per frame.  A plane is 1 024 words, word k * 32 + j holding the 32 points of one x row (bit i = x index i); thread
// t owns the words t, t + 256, t + 512 and t + 768 of every plane.
//  1. Occupancy: the receptor (the frame's pocket atoms, then the group's static atoms) goes through in tiles of 256 atoms; the
//     atoms inside the lattice's box grown by their own expanded radius are compacted into an LDS list (ballot prefixes) and every
//     listed atom is worked off by 8 threads, each taking every 8th z layer of the atom's index range: the float32 point test of
//     the specification per point, one atomicOr per x row.  Every writer ORs in ones, so order cannot matter.  The ligand likewise.
//  2. Burial, word-parallel: per word and line the hit masks of both senses are ORs of shifted P words; the 7 "both senses" masks
//     are added into three bit-sliced planes; b >= min_buried is a bitwise comparison.
//  3. Flood fill: reached = the filled points; reached |= (its 6 neighbours) & cavity until a workgroup-wide vote sees no change.
//     Words are read while their owners may be updating them: every update only adds bits of the same fixed point.
//  4. Mouth and totals by mask arithmetic and popcounts, lining with one receptor atom per thread, integer sums throughout.
// The filters only drop atoms that can mark no point, every point test is the same float32 expression, every reduction is an
// integer OR or sum: the bits of a frame do not depend on the launch.
#define CV_THREADS FR_THREADS
#define CV_WAVES FR_WAVES
#define CV_MAX_LIG 256
#define CV_MAX_POCKET 8192
#define CV_MAX_RES 16384
#define CV_WORDS 1024              // x rows of the 32^3 lattice
#define CV_OWN (CV_WORDS / CV_THREADS)
#define CV_SUB 8                   // threads per listed atom
#define CV_LO_MIN (-4096)
#define CV_LO_MAX 4064
#define CV_SLACK 0.05f             // the filters are this much wider than the widest test: beyond any rounding at |x| <= 1e4
#define CV_MAX_SWEEPS 32768        // a path through 32^3 points is shorter
#define CV_TOTALS 12

struct CvArgs {
  dbfr_cavity_in in;
  dbfr_cavity_out out;
  float h, probe, cut;
  int min_buried;
  int T[7];                        // steps per sense of the 7 lines
  uint32_t* cmask;                 // workspace: the mask of C of every frame (read by k_cavity_common), or nullptr
};

// the lattice indices (relative to lo, clamped to the box) an atom at x can reach within R: one index wider than the float32
// quotients say on either side; the point test decides.  Empty when a > b.
__device__ __forceinline__ void cv_range(float x, float R, float h, int lo, int& a, int& b) {
  const float lof = (float)lo;
  const float fa = floorf((x - R) / h) - 1.f - lof, fb = ceilf((x + R) / h) + 1.f - lof;
  a = (int)fminf(fmaxf(fa, 0.f), 32.f);
  b = (int)fminf(fmaxf(fb, -1.f), 31.f);
}

__device__ __forceinline__ uint32_t cv_bits(int a, int b) {      // bits a .. b, 0 <= a <= b <= 31
  return (0xffffffffu >> (31 - b)) & (0xffffffffu << a);
}

// the lattice points with |q - x|^2 < R2 of the z layers az + sub, az + sub + CV_SUB, ... of the atom's range
__device__ __forceinline__ void cv_mark(uint32_t* plane, float x, float y, float z, float R, float R2, float h, int lx, int ly, int lz,
                                        int sub) {
  int ax, bx, ay, by, az, bz;
  cv_range(x, R, h, lx, ax, bx);
  cv_range(y, R, h, ly, ay, by);
  cv_range(z, R, h, lz, az, bz);
  if (ax > bx || ay > by) return;
  for (int k = az + sub; k <= bz; k += CV_SUB) {
    const float dz = h * (float)(lz + k) - z, dz2 = dz * dz;
    for (int j = ay; j <= by; ++j) {
      const float dy = h * (float)(ly + j) - y, dy2 = dy * dy;
      uint32_t m = 0;
      for (int i = ax; i <= bx; ++i) {
        const float dx = h * (float)(lx + i) - x;
        if (dx * dx + dy2 + dz2 < R2) m |= 1u << i;
      }
      if (m) atomicOr(&plane[k * 32 + j], m);
    }
  }
}

__device__ __forceinline__ uint32_t cv_word(const uint32_t* plane, int k, int j) {     // a point outside the box is solvent
  return ((unsigned)k < 32u && (unsigned)j < 32u) ? plane[k * 32 + j] : 0u;
}

// bit i of the result = bit i + s of w
__device__ __forceinline__ uint32_t cv_shift(uint32_t w, int s) { return s > 0 ? w >> s : (s < 0 ? w << -s : w); }

// the points of word (k, j) whose line along (dx, dy, dz) reaches a P point within T steps in both senses
__device__ __forceinline__ uint32_t cv_line(const uint32_t* P, int k, int j, int dx, int dy, int dz, int T) {
  uint32_t fwd = 0, back = 0;
  for (int t = 1; t <= T; ++t) {
    fwd |= cv_shift(cv_word(P, k + t * dz, j + t * dy), t * dx);
    back |= cv_shift(cv_word(P, k - t * dz, j - t * dy), -t * dx);
  }
  return fwd & back;
}

__global__ __launch_bounds__(CV_THREADS) void k_pose_cavity(CvArgs a) {
  extern __shared__ uint32_t cv_res[];                      // one byte per residue column, four to a word
  __shared__ uint32_t planes[7][CV_WORDS];
  __shared__ float4 list[CV_THREADS];
  __shared__ int wcnt[CV_WAVES];
  __shared__ float redf[CV_WAVES][8];
  __shared__ int red[CV_WAVES][CV_TOTALS];
  uint32_t *P = planes[0], *LIG = planes[1], *B0 = planes[2], *B1 = planes[3], *B2 = planes[4], *CAV = planes[5], *RCH = planes[6];
  const dbfr_cavity_in& in = a.in;
  const dbfr_cavity_out& out = a.out;
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = frame_group(in.frame_ptr, in.n_group, f);
  const int kf = f - in.frame_ptr[g];
  const int n0 = in.lig_ptr[g], NL = in.lig_ptr[g + 1] - n0;
  const int m0 = in.pocket_ptr[g], M = in.pocket_ptr[g + 1] - m0;
  const int s0 = in.static_ptr ? in.static_ptr[g] : 0, S = in.static_ptr ? in.static_ptr[g + 1] - s0 : 0;
  const int NR = in.res_ptr[g + 1] - in.res_ptr[g];
  const int lx = in.grid_lo[3 * g], ly = in.grid_lo[3 * g + 1], lz = in.grid_lo[3 * g + 2];
  const bool res_ok = NR >= 0 && NR <= in.max_res;
  const bool lig_ok = NL >= 0 && NL <= in.max_lig && NL <= CV_MAX_LIG;
  const bool lo_ok = lx >= CV_LO_MIN && lx <= CV_LO_MAX && ly >= CV_LO_MIN && ly <= CV_LO_MAX && lz >= CV_LO_MIN && lz <= CV_LO_MAX;
  const bool shape_ok = res_ok && lig_ok && lo_ok && M >= 0 && M <= in.max_pocket && S >= 0;
  const int MR = shape_ok ? M + S : 0;
  const float* lp = in.lig_pos + 3 * (in.lig_pos_off[g] + (long long)kf * NL);
  Receptor rec;
  rec.pp = in.pocket_pos + 3 * (in.pocket_pos_off[g] + (long long)kf * M);
  rec.sp = in.static_pos + 3 * (size_t)s0;
  rec.prad = in.pocket_rad + m0;
  rec.srad = in.static_rad + s0;
  rec.M = M;
  const float h = a.h;
  for (int t = tid; t < 7 * CV_WORDS; t += CV_THREADS) planes[0][t] = 0u;
  if (res_ok)
    for (int t = tid; t < (NR + 3) / 4; t += CV_THREADS) cv_res[t] = 0u;
  FrameBox box;                                             // the lattice's box
  box.add(h * (float)lx, h * (float)ly, h * (float)lz, 0.f);
  box.add(h * (float)(lx + 31), h * (float)(ly + 31), h * (float)(lz + 31), 0.f);
  __syncthreads();                                          // the planes are zero
  // 1. the receptor, a tile of 256 atoms at a time
  int bad_atom = 0;
  for (int b0 = 0; b0 < MR; b0 += CV_THREADS) {
    const int b = b0 + tid;
    bool c = false;
    float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
    if (b < MR) {
      const float* y = rec.pos(b);
      e = make_float4(y[0], y[1], y[2], rec.rad(b));
      const bool ok = atom_ok(e.x, e.y, e.z, e.w);
      bad_atom |= !ok;
      c = ok && box.touches(e.x, e.y, e.z, e.w + a.probe + CV_SLACK);
    }
    int slot, sum;
    block_compact(c, 0, wcnt, lane, wave, slot, sum);
    if (c) list[slot] = e;
    __syncthreads();                                        // the entries complete; wcnt is rewritten by the next tile
    for (int w = tid; w < sum * CV_SUB; w += CV_THREADS) {
      const float4 v = list[w / CV_SUB];
      const float R = v.w + a.probe;
      cv_mark(P, v.x, v.y, v.z, R, R * R, h, lx, ly, lz, w % CV_SUB);
    }
  }
  // the ligand: the van der Waals sphere, and the atoms whose own nearest lattice point lies outside the box
  int n_outside = 0;
  if (shape_ok)
    for (int w = tid; w < NL * CV_SUB; w += CV_THREADS) {
      const int i = w / CV_SUB, sub = w % CV_SUB;
      const float x = lp[3 * (size_t)i], y = lp[3 * (size_t)i + 1], z = lp[3 * (size_t)i + 2], r = in.lig_rad[n0 + i];
      if (!atom_ok(x, y, z, r)) {
        bad_atom = 1;
        continue;
      }
      cv_mark(LIG, x, y, z, r, r * r, h, lx, ly, lz, sub);
      if (sub == 0) {
        const float ix = rintf(x / h) - (float)lx, iy = rintf(y / h) - (float)ly, iz = rintf(z / h) - (float)lz;
        n_outside += ix < 0.f || ix > 31.f || iy < 0.f || iy > 31.f || iz < 0.f || iz > 31.f;
      }
    }
  const bool bad = __syncthreads_or(bad_atom) || !shape_ok; // uniform over the workgroup; P and LIG complete
  int v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  FrameBox cbox;                                            // the box of C
  if (!bad) {
    // 2. burial and the cavity points
    for (int o = 0; o < CV_OWN; ++o) {
      const int w = tid + o * CV_THREADS, k = w >> 5, j = w & 31;
      uint32_t b0 = 0, b1 = 0, b2 = 0;
      auto add = [&](uint32_t m) {
        const uint32_t c0 = b0 & m;
        b0 ^= m;
        const uint32_t c1 = b1 & c0;
        b1 ^= c0;
        b2 |= c1;
      };
      add(cv_line(P, k, j, 1, 0, 0, a.T[0]));
      add(cv_line(P, k, j, 0, 1, 0, a.T[1]));
      add(cv_line(P, k, j, 0, 0, 1, a.T[2]));
      add(cv_line(P, k, j, 1, 1, 1, a.T[3]));
      add(cv_line(P, k, j, 1, 1, -1, a.T[4]));
      add(cv_line(P, k, j, 1, -1, 1, a.T[5]));
      add(cv_line(P, k, j, -1, 1, 1, a.T[6]));
      const uint32_t solvent = ~P[w];
      b0 &= solvent; b1 &= solvent; b2 &= solvent;
      B0[w] = b0; B1[w] = b1; B2[w] = b2;
      // b >= min_buried, from the high bit down
      const int mb = a.min_buried;
      uint32_t gt = 0, eq = 0xffffffffu;
      if (mb & 4) eq &= b2; else { gt |= eq & b2; eq &= ~b2; }
      if (mb & 2) eq &= b1; else { gt |= eq & b1; eq &= ~b1; }
      if (mb & 1) eq &= b0; else { gt |= eq & b0; eq &= ~b0; }
      const uint32_t cav = (gt | eq) & solvent;
      CAV[w] = cav;
      RCH[w] = cav & LIG[w];
    }
    // 3. flood fill: every thread reaches the vote of every sweep
    __syncthreads();                                        // the cavity points and the seeds are written
    for (int sweep = 0; sweep < CV_MAX_SWEEPS; ++sweep) {
      int changed = 0;
      for (int o = 0; o < CV_OWN; ++o) {
        const int w = tid + o * CV_THREADS, k = w >> 5, j = w & 31;
        const uint32_t cav = CAV[w], r0 = RCH[w];
        uint32_t r = (r0 | cv_word(RCH, k, j - 1) | cv_word(RCH, k, j + 1) | cv_word(RCH, k - 1, j) | cv_word(RCH, k + 1, j)) & cav;
        for (;;) {                                          // along x inside the word, to its own fixed point
          const uint32_t n = (r | (r << 1) | (r >> 1)) & cav;
          if (n == r) break;
          r = n;
        }
        if (r != r0) {
          RCH[w] = r;
          changed = 1;
        }
      }
      if (!__syncthreads_or(changed)) break;                // a barrier and the vote, uniform: the words of the sweep are written,
                                                            // and all threads leave together
    }
    // 4. mouth, totals and the box of C
    for (int o = 0; o < CV_OWN; ++o) {
      const int w = tid + o * CV_THREADS, k = w >> 5, j = w & 31;
      const uint32_t p = P[w], lig = LIG[w], cav = CAV[w], c = RCH[w], b0 = B0[w], b1 = B1[w], b2 = B2[w];
      auto open = [&](int kk, int jj) {                     // solvent and no cavity point; every point outside the box
        return ((unsigned)kk < 32u && (unsigned)jj < 32u) ? ~(P[kk * 32 + jj] | CAV[kk * 32 + jj]) : 0xffffffffu;
      };
      const uint32_t here = ~(p | cav);
      const uint32_t mouth = c & ((here << 1) | 1u | (here >> 1) | 0x80000000u | open(k, j - 1) | open(k, j + 1) | open(k - 1, j) | open(k + 1, j));
      const uint32_t fill = lig & cav;
      v[0] += __popc(lig);
      v[1] += __popc(lig & p);
      v[2] += __popc(fill);
      v[3] += __popc(lig & here);
      v[4] += __popc(c);
      v[5] += __popc(mouth);
      v[6] += __popc(b0 & c) + 2 * __popc(b1 & c) + 4 * __popc(b2 & c);
      v[7] += __popc(b0 & fill) + 2 * __popc(b1 & fill) + 4 * __popc(b2 & fill);
      if (c) {
        const float qy = h * (float)(ly + j), qz = h * (float)(lz + k);
        cbox.add(h * (float)(lx + __builtin_ctz(c)), qy, qz, 0.f);
        cbox.add(h * (float)(lx + 31 - __builtin_clz(c)), qy, qz, 0.f);
      }
    }
  }
  cbox.block_reduce(redf, lane, wave);                      // (its barrier: uniform, outside every branch)
  if (!bad) {
    // lining: one receptor atom per thread over the points of C inside its cutoff cube
    const float cut = a.cut, cut2 = cut * cut;
    for (int b = tid; b < MR; b += CV_THREADS) {
      const float* y = rec.pos(b);
      const float x = y[0], yy = y[1], z = y[2];
      if (!cbox.touches(x, yy, z, cut + CV_SLACK)) continue;
      int ax, bx, ay, by, az, bz;
      cv_range(x, cut, h, lx, ax, bx);
      cv_range(yy, cut, h, ly, ay, by);
      cv_range(z, cut, h, lz, az, bz);
      if (ax > bx) continue;
      const uint32_t span = cv_bits(ax, bx);
      int fl = 0;
      for (int k = az; k <= bz && fl != 3; ++k) {
        const float dz = h * (float)(lz + k) - z, dz2 = dz * dz;
        for (int j = ay; j <= by && fl != 3; ++j) {
          const uint32_t c = RCH[k * 32 + j] & span, room = c & ~LIG[k * 32 + j];
          uint32_t m = fl ? room : c;                       // once the atom lines C only the free room is left to find
          if (!m) continue;
          const float dy = h * (float)(ly + j) - yy, dy2 = dy * dy;
          while (m) {
            const int i = __builtin_ctz(m);
            m &= m - 1;
            const float dx = h * (float)(lx + i) - x;
            if (dx * dx + dy2 + dz2 <= cut2) fl |= 1 | (((room >> i) & 1u) << 1);
          }
        }
      }
      if (!fl) continue;
      const int col = *rec.sel(b, in.pocket_col + m0, in.static_col + s0);
      const bool polar = *rec.sel(b, in.pocket_polar + m0, in.static_polar + s0) != 0;
      if (NR > 0) {
        const int cc = min(max(col, 0), NR - 1);
        atomicOr(&cv_res[cc >> 2], (uint32_t)fl << (8 * (cc & 3)));
      }
      v[8] += 1;
      v[9] += polar;
    }
  }
  n_outside = wave_sum(n_outside);
  for (int q = 0; q < 10; ++q) {
    const int s = wave_sum(v[q]);
    if (lane == 0) red[wave][q] = s;
  }
  if (lane == 0) red[wave][10] = n_outside;
  __syncthreads();                                          // the per-wave sums and every residue byte complete
  if (res_ok && out.lining) {
    uint8_t* row = out.lining + in.res_off[g] + (long long)kf * NR;
    for (int r = tid; r < NR; r += CV_THREADS) row[r] = bad ? 0 : (uint8_t)((cv_res[r >> 2] >> (8 * (r & 3))) & 0xffu);
  }
  if (tid < CV_TOTALS && out.totals) {
    int s = -1;                                             // n_common: k_cavity_common writes it where there is a reference
    if (tid < 11) {
      s = 0;
      for (int w = 0; w < CV_WAVES; ++w) s += red[w][tid];
    }
    out.totals[CV_TOTALS * (size_t)f + tid] = bad ? -1 : s;
  }
  for (int o = 0; o < CV_OWN; ++o) {
    const int w = tid + o * CV_THREADS;
    const uint32_t c = bad ? 0u : RCH[w];
    if (a.cmask) a.cmask[CV_WORDS * (size_t)f + w] = c;
    if (out.masks) {
      out.masks[2 * CV_WORDS * (size_t)f + w] = c;
      out.masks[2 * CV_WORDS * (size_t)f + CV_WORDS + w] = bad ? 0u : c & LIG[w];
    }
    if (out.burial) {
      uint32_t* dst = reinterpret_cast<uint32_t*>(out.burial + 32 * (CV_WORDS * (size_t)f + w));
      const uint32_t b0 = bad ? 0u : B0[w], b1 = bad ? 0u : B1[w], b2 = bad ? 0u : B2[w];
      for (int q = 0; q < 8; ++q) {
        uint32_t word = 0;
        for (int i = 0; i < 4; ++i) {
          const int bit = 4 * q + i;
          word |= (((b0 >> bit) & 1u) | (((b1 >> bit) & 1u) << 1) | (((b2 >> bit) & 1u) << 2)) << (8 * i);
        }
        dst[q] = word;
      }
    }
  }
}

// |C of the frame AND C of its group's reference frame| into totals[:, 11]: one wave per frame, 16 words per lane.  -1 stays where
// the group has no reference frame, the reference is no frame of the group, or either frame is unusable.
__global__ __launch_bounds__(CV_THREADS) void k_cavity_common(dbfr_cavity_in in, const uint32_t* cmask, int32_t* totals) {
  const int f = blockIdx.x * CV_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (f >= in.n_frame) return;
  const int g = frame_group(in.frame_ptr, in.n_group, f);
  const int r = in.ref_frame[g];
  if (r < in.frame_ptr[g] || r >= in.frame_ptr[g + 1]) return;
  if (totals[CV_TOTALS * (size_t)f] < 0 || totals[CV_TOTALS * (size_t)r] < 0) return;
  int n = 0;
  for (int w = lane; w < CV_WORDS; w += 64) n += __popc(cmask[CV_WORDS * (size_t)f + w] & cmask[CV_WORDS * (size_t)r + w]);
  n = wave_sum(n);
  if (lane == 0) totals[CV_TOTALS * (size_t)f + 11] = n;
}

// ------------------------------------------------------------------------------------------------ host
static const char* CV_FN = "dbfr_pose_cavity";
static int cv_err(const std::string& s) { return arg_err(CV_FN, s); }

// the host copies of the index arrays, when the caller has them: every count, column, radius, lattice corner and reference frame
static int cv_validate(const dbfr_cavity_in& d, const dbfr_cavity_in& h) {
  if (!h.frame_ptr || !h.lig_ptr || !h.lig_rad || !h.pocket_ptr || !h.pocket_rad || !h.pocket_col || !h.res_ptr || !h.grid_lo ||
      (d.static_ptr && (!h.static_ptr || !h.static_rad || !h.static_col)) || (d.ref_frame && !h.ref_frame))
    return cv_err("host: a host copy of an index array is missing");
  const int G = d.n_group;
  if (const int rc = frame_ptr_err(CV_FN, h.frame_ptr, G, d.n_frame)) return rc;
  for (int g = 0; g < G; ++g) {
    const std::string where = "group " + std::to_string(g) + ": ";
    const int n0 = h.lig_ptr[g], NL = h.lig_ptr[g + 1] - n0, m0 = h.pocket_ptr[g], M = h.pocket_ptr[g + 1] - m0,
              s0 = d.static_ptr ? h.static_ptr[g] : 0, S = d.static_ptr ? h.static_ptr[g + 1] - s0 : 0, NR = h.res_ptr[g + 1] - h.res_ptr[g];
    if (const int rc = group_counts_err(CV_FN, where, {{h.frame_ptr[g + 1] - h.frame_ptr[g]}, {NL, "ligand atoms", "max_lig", d.max_lig},
                                                       {M, "pocket atoms", "max_pocket", d.max_pocket}, {S},
                                                       {NR, "residue columns", "max_res", d.max_res}}))
      return rc;
    for (int c = 0; c < 3; ++c)
      if (h.grid_lo[3 * g + c] < CV_LO_MIN || h.grid_lo[3 * g + c] > CV_LO_MAX)
        return limit_err(CV_FN, (where + "grid_lo").c_str(), h.grid_lo[3 * g + c], CV_LO_MIN, CV_LO_MAX);
    if (d.ref_frame && h.ref_frame[g] != -1 && (h.ref_frame[g] < h.frame_ptr[g] || h.ref_frame[g] >= h.frame_ptr[g + 1]))
      return cv_err(where + "ref_frame " + std::to_string(h.ref_frame[g]) + " is no frame of the group (" + std::to_string(h.frame_ptr[g]) +
                    " .. " + std::to_string(h.frame_ptr[g + 1] - 1) + ") and not -1");
    for (int i = 0; i < NL; ++i)
      if (!(h.lig_rad[n0 + i] > 0.f && h.lig_rad[n0 + i] <= 4.f))
        return cv_err(where + "the radius of ligand atom " + std::to_string(i) + " lies outside (0, 4]");
    if (const int rc = receptor_atoms_err(CV_FN, where, M, S, h.pocket_rad + m0, d.static_ptr ? h.static_rad + s0 : nullptr, h.pocket_col + m0,
                                          d.static_ptr ? h.static_col + s0 : nullptr, NR, [](int) { return DBFR_OK; }))
      return rc;
  }
  return DBFR_OK;
}

// the options checked (NaN fails every range) and the steps per sense of the 7 lines, in float64 of the float32 values
static int cv_opts(const dbfr_cavity_opts* opts, dbfr_cavity_opts& o, int T[7]) {
  o = {1.0f, 1.2f, 8.0f, 4.0f, 6};
  if (opts) o = *opts;
  if (!(o.spacing >= 0.75f && o.spacing <= 2.f)) return cv_err("spacing must lie in [0.75, 2] A and must not be NaN");
  if (!(o.probe >= 0.f && o.probe <= 4.f)) return cv_err("probe must lie in [0, 4] A and must not be NaN");
  if (!(o.ray_length >= o.spacing && o.ray_length <= 31.f * o.spacing)) return cv_err("ray_length must lie in [spacing, 31 spacing] and must not be NaN");
  if (!(o.lining_cutoff >= 0.f && o.lining_cutoff <= 6.f)) return cv_err("lining_cutoff must lie in [0, 6] A and must not be NaN");
  if (o.min_buried < 1 || o.min_buried > 7) return limit_err(CV_FN, "min_buried", o.min_buried, 1, 7);
  const double h = (double)o.spacing, L = (double)o.ray_length;
  for (int e = 0; e < 7; ++e) T[e] = (int)std::floor(L / (e < 3 ? h : h * std::sqrt(3.0)));
  return DBFR_OK;
}

static int cv_shape(const dbfr_cavity_in* in) {
  if (in->n_group < 0 || in->n_frame < 0) return cv_err("negative n_group / n_frame");
  if (in->max_lig < 0 || in->max_lig > CV_MAX_LIG) return limit_err(CV_FN, "max_lig (ligand atoms)", in->max_lig, 0, CV_MAX_LIG);
  if (in->max_pocket < 0 || in->max_pocket > CV_MAX_POCKET) return limit_err(CV_FN, "max_pocket (pocket atoms)", in->max_pocket, 0, CV_MAX_POCKET);
  if (in->max_res < 0 || in->max_res > CV_MAX_RES) return limit_err(CV_FN, "max_res (residue columns)", in->max_res, 0, CV_MAX_RES);
  return DBFR_OK;
}

extern "C" int dbfr_pose_cavity_workspace_bytes(const dbfr_cavity_in* in, size_t* bytes) {
  if (!in || !bytes) return cv_err("null argument");
  if (const int rc = cv_shape(in)) return rc;
  *bytes = in->ref_frame ? 4 * (size_t)CV_WORDS * (size_t)in->n_frame : 0;
  return DBFR_OK;
}

extern "C" int dbfr_pose_cavity(const dbfr_cavity_in* in, const dbfr_cavity_opts* opts, const dbfr_cavity_out* out, void* hip_stream) {
  if (!in || !out) return cv_err("null argument");
  if (const int rc = cv_shape(in)) return rc;
  CvArgs a;
  dbfr_cavity_opts o;
  if (const int rc = cv_opts(opts, o, a.T)) return rc;
  if (in->n_frame == 0) return DBFR_OK;
  if (in->n_group == 0) return cv_err("frames without groups");
  if (!in->frame_ptr || !in->lig_ptr || !in->lig_pos_off || !in->lig_pos || !in->lig_rad || !in->pocket_ptr || !in->pocket_pos_off ||
      !in->pocket_pos || !in->pocket_rad || !in->pocket_col || !in->pocket_polar || !in->res_ptr || !in->res_off || !in->grid_lo)
    return cv_err("frame_ptr / lig_ptr / lig_pos_off / lig_pos / lig_rad / pocket_ptr / pocket_pos_off / pocket_pos / pocket_rad / "
                  "pocket_col / pocket_polar / res_ptr / res_off / grid_lo missing");
  if (in->static_ptr && (!in->static_pos || !in->static_rad || !in->static_col || !in->static_polar))
    return cv_err("static_ptr given without static_pos / static_rad / static_col / static_polar");
  const size_t need = in->ref_frame ? 4 * (size_t)CV_WORDS * (size_t)in->n_frame : 0;
  if (need && (!out->workspace || out->workspace_bytes < need))
    return cv_err("ref_frame given: the workspace holds " + std::to_string(out->workspace ? out->workspace_bytes : 0) + " bytes, " +
                  std::to_string(need) + " are needed (dbfr_pose_cavity_workspace_bytes)");
  if (need && !out->totals) return cv_err("ref_frame given without totals");
  if (in->host) {
    const int rc = cv_validate(*in, *static_cast<const dbfr_cavity_in*>(in->host));
    if (rc != DBFR_OK) return rc;
  }
  a.in = *in;
  a.in.host = nullptr;
  a.out = *out;
  a.h = o.spacing;
  a.probe = o.probe;
  a.cut = o.lining_cutoff;
  a.min_buried = o.min_buried;
  a.cmask = need ? static_cast<uint32_t*>(out->workspace) : nullptr;
  const size_t lds = 4 * (((size_t)in->max_res + 3) / 4) + 16;
  HIPCHECK(launch_frames(k_pose_cavity, in->n_frame, CV_THREADS, lds, hip_stream, a));
  if (need) {
    hipLaunchKernelGGL(k_cavity_common, dim3((unsigned)((in->n_frame + CV_WAVES - 1) / CV_WAVES)), dim3(CV_THREADS), 0, (hipStream_t)hip_stream,
                       a.in, a.cmask, out->totals);
    HIPCHECK(hipGetLastError());
  }
  return DBFR_OK;
}
