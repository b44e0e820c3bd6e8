// Validity checks of each pose's own sampled pocket: steric clashes of the movable side-chain atoms against the rest of the
// receptor and the lengths of the bonds a chi rotation can break, for every frame of a ragged batch, in one launch.
// include/dbfr.h states the definitions; docs/pocketcheck.md the layout and the limits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/dbfr.h"
#include "common.h"
#include "frames.h"

// One workgroup per frame.  The frame's MOVABLE atoms (x, y, z, r) are staged in LDS in list order, with their bounding box.
// The partners (pocket atoms of the frame, then the static atoms of the group) stream past in tiles of one atom per thread: a
// pocket atom is always a candidate, a static atom only inside the box grown by the largest distance at which its ratio to any
// movable atom can stay below cap = max(clash_ratio, 1).  Candidates are compacted in index order by ballot prefixes into an LDS
// list; a full list is worked off one candidate per thread against the movable atoms in LDS (every lane reads the same movable
// atom: a broadcast).  A movable partner of list position j meets only the movable atoms before it, so that a pair of two
// movable atoms is seen once.  A squared-distance filter against the thread's running threshold comes first; the ratio, the
// exclusion list (memory) and the residue columns are touched only by the pairs that pass it.  That fast pass is exact whenever
// the frame has a pair below cap; a frame without one (nothing near its side chains) takes a second pass over every partner
// without any filter.  Every reduction is a minimum over (ratio, a, b) keys, a maximum or an integer count, and the per-residue
// bytes saturate: the bits of a frame do not depend on the launch it is part of.
#define PK_THREADS FR_THREADS
#define PK_WAVES FR_WAVES
#define PK_MAX_POCKET 8192
#define PK_MAX_EXCL 32
#define PK_MAX_RES 16384
#define PK_CAND 1024               // candidate list (4 KB)
#define PK_SLACK 1.000005f         // the squared-distance filter is wider than the ratio test by this factor

struct PkArgs {
  dbfr_pocket_check_in in;
  dbfr_pocket_check_opts o;
  dbfr_pocket_check_out out;
  int cap;                         // candidate list length in use
  int lds_mov;                     // float4 slots of the dynamic LDS that hold movable atoms; the residue bytes follow
};

struct PkKey {                     // the worst pair so far: smallest ratio, ties to the lexicographically smallest (a, b)
  float r;
  int a, b;
};

__device__ __forceinline__ bool key_less(float r, int a, int b, const PkKey& k) {
  return r < k.r || (r == k.r && (a < k.a || (a == k.a && b < k.b)));
}

// saturating +1 on byte `col` of the packed residue counters (rare: only clashing pairs come here)
__device__ __forceinline__ void bump(unsigned* resw, int col) {
  const int sh = 8 * (col & 3);
  unsigned old = resw[col >> 2];
  while (((old >> sh) & 255u) != 255u) {
    const unsigned seen = atomicCAS(&resw[col >> 2], old, old + (1u << sh));
    if (seen == old) break;
    old = seen;
  }
}

struct PkFrame {                   // what a pair needs of its frame and group
  const float4* mx;
  unsigned* resw;
  const int32_t *mov_atom, *excl_ptr, *excl, *pocket_col;
  int M, NMOV, NR;
  float clash, cap;
};

// Partner b (receptor atom index; position, radius, column, list position or -1, category) against the movable atoms.
// FULL: no filter and no counting (the second pass of a frame that has no pair below cap).
template <bool FULL>
__device__ __forceinline__ void scan_partner(const PkFrame& fr, int b, float bx, float by, float bz, float rb, int colb, int rankb,
                                             int cat, PkKey& key, float& thr, int (&n)[3]) {
  const int iend = rankb >= 0 ? min(rankb, fr.NMOV) : fr.NMOV;
  for (int i = 0; i < iend; ++i) {
    const float4 q = fr.mx[i];
    const float dx = q.x - bx, dy = q.y - by, dz = q.z - bz;
    const float d2 = dx * dx + dy * dy + dz * dz;
    const float s = q.w + rb;
    if (!FULL) {
      const float lim = s * thr;
      if (!(d2 < lim * lim)) continue;
    }
    const float ratio = sqrtf(d2) / s;
    if (!FULL && !(ratio < fr.cap)) continue;
    const bool clashing = !FULL && ratio < fr.clash;
    if (!(clashing || ratio <= key.r)) continue;
    const int e0 = fr.excl_ptr[i], ne = min(max(fr.excl_ptr[i + 1] - e0, 0), PK_MAX_EXCL);
    bool excluded = false;
    for (int e = 0; e < ne; ++e) excluded = excluded || fr.excl[e0 + e] == b;
    if (excluded) continue;
    const int ai = min(max(fr.mov_atom[i], 0), fr.M - 1);
    const int lo = min(ai, b), hi = max(ai, b);
    if (key_less(ratio, lo, hi, key)) {
      key.r = ratio; key.a = lo; key.b = hi;
      if (!FULL) thr = fmaxf(fr.clash, fminf(ratio, fr.cap)) * PK_SLACK;
    }
    if (clashing) {
      ++n[cat];
      if (fr.NR > 0) {
        const int cola = min(max(fr.pocket_col[ai], 0), fr.NR - 1), cb = min(max(colb, 0), fr.NR - 1);
        bump(fr.resw, cola);
        if (cb != cola) bump(fr.resw, cb);
      }
    }
  }
}

// the smallest key of the workgroup, in every thread (two barriers)
__device__ __forceinline__ PkKey block_min_key(PkKey k, float (*redf)[8], int (*redi)[8], int lane, int wave) {
  for (int o = 32; o > 0; o >>= 1) {
    const float r = __shfl_xor(k.r, o);
    const int a = __shfl_xor(k.a, o), b = __shfl_xor(k.b, o);
    if (key_less(r, a, b, k)) { k.r = r; k.a = a; k.b = b; }
  }
  if (lane == 0) { redf[wave][7] = k.r; redi[wave][6] = k.a; redi[wave][7] = k.b; }
  __syncthreads();
  k.r = redf[0][7]; k.a = redi[0][6]; k.b = redi[0][7];
  for (int w = 1; w < PK_WAVES; ++w)
    if (key_less(redf[w][7], redi[w][6], redi[w][7], k)) { k.r = redf[w][7]; k.a = redi[w][6]; k.b = redi[w][7]; }
  __syncthreads();
  return k;
}

__global__ __launch_bounds__(PK_THREADS) void k_pocket_check(PkArgs a) {
  extern __shared__ float4 pk_dyn[];                        // movable atoms (x, y, z, r), then one byte per residue column
  __shared__ int cand[PK_CAND];
  __shared__ int wcnt[PK_WAVES];
  __shared__ float redf[PK_WAVES][8];
  __shared__ int redi[PK_WAVES][8];
  const dbfr_pocket_check_in& in = a.in;
  const dbfr_pocket_check_out& out = a.out;
  float4* mx = pk_dyn;
  unsigned* resw = reinterpret_cast<unsigned*>(pk_dyn + a.lds_mov);
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = frame_group(in.frame_ptr, in.n_group, f);
  const int k = f - in.frame_ptr[g];
  const int m0 = in.pocket_ptr[g], M = in.pocket_ptr[g + 1] - m0;
  const int s0 = in.static_ptr ? in.static_ptr[g] : 0, S = in.static_ptr ? in.static_ptr[g + 1] - s0 : 0;
  const int v0 = in.mov_ptr[g], NMOV = in.mov_ptr[g + 1] - v0;
  const int c0 = in.closure_ptr[g], NC = in.closure_ptr[g + 1] - c0;
  const int NR = in.res_ptr[g + 1] - in.res_ptr[g];
  const bool res_ok = NR >= 0 && NR <= in.max_res;
  const bool shape_ok = res_ok && M >= 0 && M <= in.max_pocket && S >= 0 && NMOV >= 0 && NMOV <= M && NC >= 0;
  const float clash = a.o.clash_ratio, cap = fmaxf(clash, 1.f);
  const int MR = shape_ok ? M + S : 0;
  const float* pp = in.pocket_pos + 3 * (in.pocket_pos_off[g] + (long long)k * M);
  const Receptor rec = {pp, in.static_pos + 3 * (size_t)s0, in.pocket_rad + m0, in.static_rad + s0, M};
  int bad_atom = 0;
  if (res_ok)
    for (int t = tid; t < (NR + 3) / 4; t += PK_THREADS) resw[t] = 0u;
  // the movable atoms and their bounding box
  FrameBox box;
  if (shape_ok)
    for (int i = tid; i < NMOV; i += PK_THREADS) {
      const int at = min(max(in.mov_atom[v0 + i], 0), M - 1);
      const float x = pp[3 * (size_t)at], y = pp[3 * (size_t)at + 1], z = pp[3 * (size_t)at + 2], r = in.pocket_rad[m0 + at];
      mx[i] = make_float4(x, y, z, r);
      box.add(x, y, z, r);
    }
  box.block_reduce(redf, lane, wave);                       // (its barrier: mx and resw complete too)
  PkFrame fr;
  fr.mx = mx; fr.resw = resw; fr.mov_atom = in.mov_atom + v0; fr.excl_ptr = in.excl_ptr + v0; fr.excl = in.excl;
  fr.pocket_col = in.pocket_col + m0; fr.M = M; fr.NMOV = shape_ok ? NMOV : 0; fr.NR = NR; fr.clash = clash; fr.cap = cap;
  PkKey key = {INFINITY, -1, -1};
  float thr = cap * PK_SLACK;
  int n[3] = {0, 0, 0};
  // fast pass: tiles of partners, candidates compacted in index order, a full list worked off
  int ncand = 0;
  for (int b0 = 0; b0 < MR; b0 += PK_THREADS) {
    const int b = b0 + tid;
    bool c = false;
    if (b < MR) {
      const float* y = rec.pos(b);
      const float bx = y[0], by = y[1], bz = y[2];
      const float rb = rec.rad(b);
      bad_atom |= !atom_ok(bx, by, bz, rb);
      const float grow = cap * (rb + box.rmax) * 1.00001f + 1e-3f;
      c = b < M || box.touches(bx, by, bz, grow);
    }
    int slot, tot;
    block_compact(c, ncand, wcnt, lane, wave, slot, tot);
    if (c) cand[slot] = b;                                  // slot < ncand + 256 <= cap: a full list is worked off in time (below)
    ncand += tot;
    __syncthreads();                                        // cand complete; wcnt is rewritten by the next tile
    if (ncand + PK_THREADS > a.cap || b0 + PK_THREADS >= MR) {
      for (int t = tid; t < ncand; t += PK_THREADS) {
        const int bb = cand[t];
        const float* y = rec.pos(bb);
        const float rb = rec.rad(bb);
        const int colb = *rec.sel(bb, in.pocket_col + m0, in.static_col + s0);
        const int rankb = bb < M ? in.pocket_rank[m0 + bb] : -1;
        scan_partner<false>(fr, bb, y[0], y[1], y[2], rb, colb, rankb, bb < M ? (rankb >= 0 ? 0 : 1) : 2, key, thr, n);
      }
      ncand = 0;
      __syncthreads();                                      // cand is rewritten by the next tile
    }
  }
  const bool bad = __syncthreads_or(bad_atom) || !shape_ok; // uniform over the workgroup
  key = block_min_key(key, redf, redi, lane, wave);
  if (!bad && key.a < 0 && fr.NMOV > 0) {                     // no pair below cap: every partner, no filter (uniform branch)
    for (int b = tid; b < MR; b += PK_THREADS) {
      const float* y = rec.pos(b);
      const float rb = rec.rad(b);
      const int rankb = b < M ? in.pocket_rank[m0 + b] : -1;
      scan_partner<true>(fr, b, y[0], y[1], y[2], rb, 0, rankb, 0, key, thr, n);
    }
    key = block_min_key(key, redf, redi, lane, wave);
  }
  // closure bonds
  int nbroken = 0;
  float maxdev = 0.f;
  if (MR > 0)
    for (int t = tid; t < NC; t += PK_THREADS) {
      const int ia = min(max(in.closure_ab[2 * (size_t)(c0 + t)], 0), MR - 1), ib = min(max(in.closure_ab[2 * (size_t)(c0 + t) + 1], 0), MR - 1);
      const float *p = rec.pos(ia), *q = rec.pos(ib);
      const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
      const float dev = fabsf(sqrtf(dx * dx + dy * dy + dz * dz) - in.closure_len[c0 + t]);
      nbroken += dev > a.o.bond_tol;
      maxdev = fmaxf(maxdev, dev);
    }
  maxdev = wave_max(maxdev);
  nbroken = wave_sum(nbroken);
  n[0] = wave_sum(n[0]); n[1] = wave_sum(n[1]); n[2] = wave_sum(n[2]);
  if (lane == 0) {
    redf[wave][0] = maxdev;
    redi[wave][0] = n[0]; redi[wave][1] = n[1]; redi[wave][2] = n[2]; redi[wave][3] = nbroken;
  }
  __syncthreads();                                          // the per-wave sums and every residue byte complete
  if (res_ok && out.res_clash) {
    uint8_t* row = out.res_clash + in.res_off[g] + (long long)k * NR;
    for (int r = tid; r < NR; r += PK_THREADS) row[r] = bad ? (uint8_t)0 : (uint8_t)((resw[r >> 2] >> (8 * (r & 3))) & 255u);
  }
  if (tid == 0) {
    for (int w = 1; w < PK_WAVES; ++w) {
      maxdev = fmaxf(maxdev, redf[w][0]);
      n[0] += redi[w][0]; n[1] += redi[w][1]; n[2] += redi[w][2]; nbroken += redi[w][3];
    }
    int pass = 0;
    pass |= ((long long)n[0] + n[1] + n[2] <= (long long)a.o.max_clashes) << 0;
    pass |= (nbroken == 0) << 1;
    pass |= (pass == 3) << 2;
    if (out.n_clash)
      for (int q = 0; q < 3; ++q) out.n_clash[3 * (size_t)f + q] = bad ? -1 : n[q];
    if (out.min_ratio) out.min_ratio[f] = bad ? NAN : key.r;
    if (out.worst_pair) {
      out.worst_pair[2 * (size_t)f] = bad ? -1 : key.a;
      out.worst_pair[2 * (size_t)f + 1] = bad ? -1 : key.b;
    }
    if (out.n_broken) out.n_broken[f] = bad ? -1 : nbroken;
    if (out.max_bond_dev) out.max_bond_dev[f] = bad ? NAN : maxdev;
    if (out.passed) out.passed[f] = bad ? 0 : pass;
  }
}

// ------------------------------------------------------------------------------------------------ host
static int pk_err(const std::string& s) { return arg_err("dbfr_pocket_check", s); }

// the host copies of the index arrays, when the caller has them: every list length, atom index, column and radius
static int pk_validate(const dbfr_pocket_check_in& d, const dbfr_pocket_check_in& h) {
  if (!h.frame_ptr || !h.pocket_ptr || !h.pocket_rad || !h.pocket_col || !h.pocket_rank || !h.mov_ptr || !h.mov_atom || !h.excl_ptr ||
      !h.excl || !h.closure_ptr || !h.closure_ab || !h.closure_len || !h.res_ptr || (d.static_ptr && (!h.static_ptr || !h.static_rad || !h.static_col)))
    return pk_err("host: a host copy of an index array is missing");
  const int G = d.n_group;
  const char* fn = "dbfr_pocket_check";
  if (const int rc = frame_ptr_err(fn, h.frame_ptr, G, d.n_frame)) return rc;
  for (int g = 0; g < G; ++g) {
    const std::string where = "group " + std::to_string(g) + ": ";
    const int m0 = h.pocket_ptr[g], M = h.pocket_ptr[g + 1] - m0, s0 = d.static_ptr ? h.static_ptr[g] : 0,
              S = d.static_ptr ? h.static_ptr[g + 1] - s0 : 0, v0 = h.mov_ptr[g], NMOV = h.mov_ptr[g + 1] - v0, c0 = h.closure_ptr[g],
              NC = h.closure_ptr[g + 1] - c0, NR = h.res_ptr[g + 1] - h.res_ptr[g];
    if (const int rc = group_counts_err(fn, where, {{h.frame_ptr[g + 1] - h.frame_ptr[g]}, {M, "pocket atoms", "max_pocket", d.max_pocket}, {S},
                                                    {NMOV}, {NC}, {NR, "residue columns", "max_res", d.max_res}}))
      return rc;
    if (NMOV > M) return pk_err(where + "more movable atoms than pocket atoms");
    const int MR = M + S;
    if (const int rc = receptor_atoms_err(fn, where, M, S, h.pocket_rad + m0, d.static_ptr ? h.static_rad + s0 : nullptr, h.pocket_col + m0,
                                          d.static_ptr ? h.static_col + s0 : nullptr, NR, [](int) { return DBFR_OK; }))
      return rc;
    int n_rank = 0;
    for (int b = 0; b < M; ++b) {
      const int rk = h.pocket_rank[m0 + b];
      if (rk < -1 || rk >= NMOV || (rk >= 0 && h.mov_atom[v0 + rk] != b))
        return pk_err(where + "pocket_rank of atom " + std::to_string(b) + " does not name its place in the movable list (index out of range)");
      n_rank += rk >= 0;
    }
    if (n_rank != NMOV) return pk_err(where + "the movable list and pocket_rank disagree");
    for (int i = 0; i < NMOV; ++i) {
      const int at = h.mov_atom[v0 + i];
      if (at < 0 || at >= M || (i > 0 && at <= h.mov_atom[v0 + i - 1]))
        return pk_err(where + "movable atom index " + std::to_string(at) + " out of range or not ascending");
      const int e0 = h.excl_ptr[v0 + i], ne = h.excl_ptr[v0 + i + 1] - e0;
      if (e0 < 0 || ne < 0) return pk_err(where + "excl_ptr does not ascend");
      if (ne > PK_MAX_EXCL)
        return pk_err(where + "an exclusion list of " + std::to_string(ne) + " atoms, at most " + std::to_string(PK_MAX_EXCL));
      for (int e = 0; e < ne; ++e) {
        const int b = h.excl[e0 + e];
        if (b < 0 || b >= MR || (e > 0 && b <= h.excl[e0 + e - 1]))
          return pk_err(where + "exclusion list atom index " + std::to_string(b) + " out of range or not ascending");
      }
    }
    for (int t = 0; t < NC; ++t) {
      const int ia = h.closure_ab[2 * (size_t)(c0 + t)], ib = h.closure_ab[2 * (size_t)(c0 + t) + 1];
      if (ia < 0 || ia >= MR || ib < 0 || ib >= MR || ia == ib)
        return pk_err(where + "closure bond atom index out of range: " + std::to_string(ia) + ", " + std::to_string(ib));
      if (!(h.closure_len[c0 + t] > 0.f && h.closure_len[c0 + t] <= 100.f)) return pk_err(where + "a closure bond length outside (0, 100] A");
    }
  }
  return DBFR_OK;
}

extern "C" int dbfr_pocket_check(const dbfr_pocket_check_in* in, const dbfr_pocket_check_opts* opts, const dbfr_pocket_check_out* out,
                                 void* hip_stream) {
  if (!in || !out) return pk_err("null argument");
  if (in->n_group < 0 || in->n_frame < 0) return pk_err("negative n_group / n_frame");
  if (in->max_pocket < 0 || in->max_pocket > PK_MAX_POCKET) return limit_err("dbfr_pocket_check", "max_pocket (pocket atoms)", in->max_pocket, 0, PK_MAX_POCKET);
  if (in->max_excl < 0 || in->max_excl > PK_MAX_EXCL) return limit_err("dbfr_pocket_check", "max_excl (exclusion list length)", in->max_excl, 0, PK_MAX_EXCL);
  if (in->max_res < 0 || in->max_res > PK_MAX_RES) return limit_err("dbfr_pocket_check", "max_res (residue columns)", in->max_res, 0, PK_MAX_RES);
  if (in->cand_cap != 0 && (in->cand_cap < PK_THREADS || in->cand_cap > PK_CAND))
    return limit_err("dbfr_pocket_check", "cand_cap (LDS partner candidates)", in->cand_cap, PK_THREADS, PK_CAND);
  dbfr_pocket_check_opts o = {0.75f, 0.3f, 0};
  if (opts) o = *opts;
  if (!(o.clash_ratio > 0.f && o.clash_ratio <= 10.f)) return pk_err("clash_ratio must lie in (0, 10] and must not be NaN");
  if (!(o.bond_tol >= 0.f && o.bond_tol <= 100.f)) return pk_err("bond_tol must lie in [0, 100] A and must not be NaN");
  if (o.max_clashes < 0) return pk_err("max_clashes must not be negative");
  if (in->n_frame == 0) return DBFR_OK;
  if (in->n_group == 0) return pk_err("frames without groups");
  if (!in->frame_ptr || !in->pocket_ptr || !in->pocket_pos_off || !in->pocket_pos || !in->pocket_rad || !in->pocket_col || !in->pocket_rank ||
      !in->mov_ptr || !in->mov_atom || !in->excl_ptr || !in->excl || !in->closure_ptr || !in->closure_ab || !in->closure_len ||
      !in->res_ptr || !in->res_off)
    return pk_err("frame_ptr / pocket_ptr / pocket_pos_off / pocket_pos / pocket_rad / pocket_col / pocket_rank / mov_ptr / mov_atom / "
                  "excl_ptr / excl / closure_ptr / closure_ab / closure_len / res_ptr / res_off missing");
  if (in->static_ptr && (!in->static_pos || !in->static_rad || !in->static_col))
    return pk_err("static_ptr given without static_pos / static_rad / static_col");
  if (in->host) {
    const int rc = pk_validate(*in, *static_cast<const dbfr_pocket_check_in*>(in->host));
    if (rc != DBFR_OK) return rc;
  }
  PkArgs a;
  a.in = *in;
  a.in.host = nullptr;
  a.o = o;
  a.out = *out;
  a.cap = in->cand_cap ? in->cand_cap : PK_CAND;
  a.lds_mov = in->max_pocket;
  const size_t lds = 16 * (size_t)in->max_pocket + 4 * (size_t)((in->max_res + 3) / 4) + 16;
  HIPCHECK(launch_frames(k_pocket_check, in->n_frame, PK_THREADS, lds, hip_stream, a));
  return DBFR_OK;
}
