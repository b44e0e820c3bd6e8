// Solvent-accessible and buried surface area of poses: Shrake-Rupley point counts of the ligand alone, the ligand in the complex
// and the receptor surface the ligand covers, for every frame of a ragged batch, in one launch.
// include/dbfr.h states the definitions; docs/sasa.md the layout and the limits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/dbfr.h"
#include "common.h"
#include "frames.h"

// One workgroup per frame.  The ligand (x, y, z, R = r + probe) and the unit vectors sit in LDS.  Two passes over the receptor
// (the frame's pocket atoms, then the group's static atoms): the first finds the largest R of an atom that can touch the ligand
// (inside the ligand's box grown by R_lmax + R_b), the second compacts, in index order by ballot prefixes, every atom that can
// touch the ligand or be the neighbour of an atom that does (inside the box grown by R_lmax + 2 R_cmax + R_c) into an LDS list of
// `cap` entries.  The list stops at the first tile of 256 atoms that no longer fits: the atoms from that tile on are read from
// memory wherever the list is read ("the sequence" = the list, then those atoms).
// Then one wave per atom, lanes over points, 64 per pass: the ligand atoms first, then every atom of the sequence.  A wave reads
// 64 possible neighbours one per lane, keeps those whose spheres meet (a margin wider than any rounding of the point test) by a
// ballot and walks the set bits: the neighbour is wave-uniform, so a lane tests its own point against a broadcast.  It leaves a
// loop when no lane is open any more.  A receptor atom's points go against the ligand first: most fail there.
// The filters only drop atoms that bury no point, every point test is the same float32 expression wherever the neighbour came
// from, and every reduction is an integer sum: the bits of a frame do not depend on the launch or on `cap`.
#define SA_THREADS FR_THREADS
#define SA_WAVES FR_WAVES
#define SA_MAX_LIG 256
#define SA_MAX_POCKET 8192
#define SA_MAX_RES 16384
#define SA_MAX_POINTS 512
#define SA_CAND 1536               // list entries by default (30 KB)
#define SA_CAND_MAX 2048
#define SA_MAX_WN (1 << 21)        // n_points * w: an int32 residue sum over 37 atoms cannot overflow
#define SA_WIDE 1.00001f           // spheres "meet" below (R_i + R_c)^2 * SA_WIDE + SA_PAD: wider than the point test can round
#define SA_PAD 1e-3f

struct SaArgs {
  dbfr_sasa_in in;
  dbfr_sasa_out out;
  float probe;
  int cap;                         // list entries in use
};

struct SaFrame {                   // what a wave needs of its frame
  const float4* lig;               // LDS
  const float4* nl;                // LDS list (x, y, z, R)
  const int* nidx;                 // LDS: receptor atom index of every list entry
  const float *pp, *sp, *prad, *srad;
  int NL, nN, M, MR, b_over, nseq;
  float probe;
};

// entry t of the sequence (per lane); false beyond its end
__device__ __forceinline__ bool sa_fetch(const SaFrame& fr, int t, float4& c, int& idx) {
  if (t < fr.nN) {
    c = fr.nl[t];
    idx = fr.nidx[t];
    return true;
  }
  const int b = fr.b_over + (t - fr.nN);
  if (b >= fr.MR) return false;
  const float* y = b < fr.M ? fr.pp + 3 * (size_t)b : fr.sp + 3 * (size_t)(b - fr.M);
  const float r = b < fr.M ? fr.prad[b] : fr.srad[b - fr.M];
  c = make_float4(y[0], y[1], y[2], r + fr.probe);
  idx = b;
  return true;
}

__device__ __forceinline__ bool sa_meet(const float4& i, const float4& c) {
  const float dx = i.x - c.x, dy = i.y - c.y, dz = i.z - c.z, s = i.w + c.w;
  return dx * dx + dy * dy + dz * dz < s * s * SA_WIDE + SA_PAD;
}

// point u of atom i buried by atom c: the difference of the centres first, never an absolute point position
__device__ __forceinline__ bool sa_buried(const float4& i, const float4& u, const float4& c) {
  const float dx = i.x - c.x, dy = i.y - c.y, dz = i.z - c.z;
  const float qx = dx + i.w * u.x, qy = dy + i.w * u.y, qz = dz + i.w * u.z;
  return qx * qx + qy * qy + qz * qz < c.w * c.w;
}

// does the sphere of atom i meet that of any ligand atom but `self` (wave-uniform)
__device__ __forceinline__ bool sa_touches_lig(const SaFrame& fr, const float4& i, int self, int lane) {
  for (int base = 0; base < fr.NL; base += 64) {
    const int t = base + lane;
    const bool meet = t < fr.NL && t != self && sa_meet(i, fr.lig[t]);
    if (__ballot(meet)) return true;
  }
  return false;
}

// per lane: is point u of atom i buried by a ligand atom other than `self`; lanes without `want` answer false
__device__ __forceinline__ bool sa_scan_lig(const SaFrame& fr, const float4& i, const float4& u, int self, bool want, int lane) {
  bool bur = false;
  for (int base = 0; base < fr.NL; base += 64) {
    const int t = base + lane;
    const bool meet = t < fr.NL && t != self && sa_meet(i, fr.lig[t]);
    unsigned long long m = __ballot(meet);
    while (m) {
      const int j = __builtin_ctzll(m);
      m &= m - 1;
      const float4 c = fr.lig[base + j];                    // every lane reads the same entry: a broadcast
      if (want && !bur) bur = sa_buried(i, u, c);
      if (!__ballot(want && !bur)) return bur;
    }
  }
  return bur;
}

// the same against the receptor atoms of the sequence
__device__ __forceinline__ bool sa_scan_rec(const SaFrame& fr, const float4& i, const float4& u, int self, bool want, int lane) {
  bool bur = false;
  for (int base = 0; base < fr.nseq; base += 64) {
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    int idx = -1;
    const bool ok = sa_fetch(fr, base + lane, c, idx);
    const bool meet = ok && idx != self && sa_meet(i, c);
    unsigned long long m = __ballot(meet);
    while (m) {
      const int j = __builtin_ctzll(m);
      m &= m - 1;
      const float4 cj = make_float4(__shfl(c.x, j), __shfl(c.y, j), __shfl(c.z, j), __shfl(c.w, j));
      if (want && !bur) bur = sa_buried(i, u, cj);
      if (!__ballot(want && !bur)) return bur;
    }
  }
  return bur;
}

__global__ __launch_bounds__(SA_THREADS) void k_sasa(SaArgs a) {
  extern __shared__ float4 sa_dyn[];                        // the list (float4, then its atom indices), then one int per residue column
  __shared__ float4 lig[SA_MAX_LIG];
  __shared__ float4 pts[SA_MAX_POINTS];
  __shared__ int wcnt[SA_WAVES];
  __shared__ float redf[SA_WAVES][8];
  __shared__ long long tot[SA_WAVES][6];
  const dbfr_sasa_in& in = a.in;
  const dbfr_sasa_out& out = a.out;
  float4* nl = sa_dyn;
  int* nidx = reinterpret_cast<int*>(sa_dyn + a.cap);
  int* res = nidx + a.cap;
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = frame_group(in.frame_ptr, in.n_group, f);
  const int k = f - in.frame_ptr[g];
  const int n0 = in.lig_ptr[g], NL = in.lig_ptr[g + 1] - n0;
  const int m0 = in.pocket_ptr[g], M = in.pocket_ptr[g + 1] - m0;
  const int s0 = in.static_ptr ? in.static_ptr[g] : 0, S = in.static_ptr ? in.static_ptr[g + 1] - s0 : 0;
  const int NR = in.res_ptr[g + 1] - in.res_ptr[g];
  const int NP = in.n_points;
  const bool res_ok = NR >= 0 && NR <= in.max_res;
  const bool lig_ok = NL >= 0 && NL <= in.max_lig && NL <= SA_MAX_LIG;
  const bool shape_ok = res_ok && lig_ok && M >= 0 && M <= in.max_pocket && S >= 0;
  const int MR = shape_ok ? M + S : 0;
  const long long lrow = in.lig_pos_off[g] + (long long)k * NL;
  const float* lp = in.lig_pos + 3 * lrow;
  const float* pp = in.pocket_pos + 3 * (in.pocket_pos_off[g] + (long long)k * M);
  const float* sp = in.static_pos + 3 * (size_t)s0;
  const float* prad = in.pocket_rad + m0;
  const float* srad = in.static_rad + s0;
  int bad_atom = 0;
  if (res_ok)
    for (int t = tid; t < NR; t += SA_THREADS) res[t] = 0;
  for (int t = tid; t < NP; t += SA_THREADS) pts[t] = make_float4(in.points[3 * t], in.points[3 * t + 1], in.points[3 * t + 2], 0.f);
  // the ligand and its bounding box
  FrameBox box;                                             // rmax: the largest R of the ligand
  if (shape_ok)
    for (int i = tid; i < NL; i += SA_THREADS) {
      const float x = lp[3 * (size_t)i], y = lp[3 * (size_t)i + 1], z = lp[3 * (size_t)i + 2], r = in.lig_rad[n0 + i];
      bad_atom |= !atom_ok(x, y, z, r);
      const float R = r + a.probe;
      lig[i] = make_float4(x, y, z, R);
      box.add(x, y, z, R);
    }
  box.block_reduce(redf, lane, wave);                       // (its barrier: lig, pts and res complete too)
  const float rlmax = box.rmax;
  // first pass: every coordinate and radius checked; the largest R of an atom that can touch the ligand
  float rcmax = 0.f;
  for (int b = tid; b < MR; b += SA_THREADS) {
    const float* y = b < M ? pp + 3 * (size_t)b : sp + 3 * (size_t)(b - M);
    const float bx = y[0], by = y[1], bz = y[2], rb = b < M ? prad[b] : srad[b - M];
    bad_atom |= !atom_ok(bx, by, bz, rb);
    const float R = rb + a.probe, grow = (rlmax + R) * SA_WIDE + 0.05f;
    if (box.touches(bx, by, bz, grow)) rcmax = fmaxf(rcmax, R);
  }
  rcmax = wave_max(rcmax);
  if (lane == 0) redf[wave][7] = rcmax;
  const bool bad = __syncthreads_or(bad_atom) || !shape_ok; // uniform over the workgroup; redf[][7] complete
  for (int w = 0; w < SA_WAVES; ++w) rcmax = fmaxf(rcmax, redf[w][7]);
  // second pass: the list, in index order
  int nN = 0, b_over = MR;
  if (!bad)
    for (int b0 = 0; b0 < MR; b0 += SA_THREADS) {
      const int b = b0 + tid;
      bool c = false;
      float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
      if (b < MR) {
        const float* y = b < M ? pp + 3 * (size_t)b : sp + 3 * (size_t)(b - M);
        e = make_float4(y[0], y[1], y[2], (b < M ? prad[b] : srad[b - M]) + a.probe);
        const float grow = (rlmax + 2.f * rcmax + e.w) * SA_WIDE + 0.1f;
        c = box.touches(e.x, e.y, e.z, grow);
      }
      int slot, sum;
      block_compact(c, nN, wcnt, lane, wave, slot, sum);
      const bool fits = nN + sum <= a.cap;                  // uniform; a tile that does not fit ends the list: memory from here on
      if (fits && c) {
        nl[slot] = e;
        nidx[slot] = b;
      }
      __syncthreads();                                      // the entries complete; wcnt is rewritten by the next tile
      if (!fits) {
        b_over = b0;                                        // this tile and every later atom: from memory
        break;
      }
      nN += sum;
    }
  SaFrame fr;
  fr.lig = lig; fr.nl = nl; fr.nidx = nidx; fr.pp = pp; fr.sp = sp; fr.prad = prad; fr.srad = srad;
  fr.NL = NL; fr.nN = nN; fr.M = M; fr.MR = MR; fr.b_over = b_over; fr.nseq = nN + (MR - b_over); fr.probe = a.probe;
  long long sum[6] = {0, 0, 0, 0, 0, 0};
  if (!bad) {
    // the ligand atoms, one per wave
    for (int i = wave; i < NL; i += SA_WAVES) {
      const float4 xi = lig[i];
      int nfree = 0, nbound = 0;
      for (int p = 0; p < NP; p += 64) {
        const float4 u = pts[p + lane];
        bool open = !sa_scan_lig(fr, xi, u, i, true, lane);
        const unsigned long long fm = __ballot(open);
        nfree += __popcll(fm);
        if (fm) {
          const bool covered = sa_scan_rec(fr, xi, u, -1, open, lane);    // every lane calls it: its lanes fetch the neighbours
          open = open && !covered;
          nbound += __popcll(__ballot(open));
        }
      }
      const long long w = in.lig_w[n0 + i];
      const bool polar = in.lig_polar[n0 + i] != 0;
      if (lane == 0) {
        if (out.lig_free) out.lig_free[lrow + i] = nfree;
        if (out.lig_bound) out.lig_bound[lrow + i] = nbound;
      }
      sum[0] += nfree * w; sum[1] += nbound * w;
      if (polar) { sum[2] += nfree * w; sum[3] += nbound * w; }
    }
    // the receptor atoms of the sequence, one per wave
    for (int t = wave; t < fr.nseq; t += SA_WAVES) {
      float4 xb = make_float4(0.f, 0.f, 0.f, 0.f);
      int b = -1;
      sa_fetch(fr, t, xb, b);                               // t < nseq: the entry exists
      if (!sa_touches_lig(fr, xb, -1, lane)) continue;
      int cnt = 0;
      for (int p = 0; p < NP; p += 64) {
        const float4 u = pts[p + lane];
        const bool hit = sa_scan_lig(fr, xb, u, -1, true, lane);
        if (!__ballot(hit)) continue;
        const bool covered = sa_scan_rec(fr, xb, u, b, hit, lane);        // every lane calls it (no short-circuit around it)
        cnt += __popcll(__ballot(hit && !covered));
      }
      if (cnt == 0) continue;
      const int w = b < M ? in.pocket_w[m0 + b] : in.static_w[s0 + (b - M)];
      const int col = b < M ? in.pocket_col[m0 + b] : in.static_col[s0 + (b - M)];
      const bool polar = (b < M ? in.pocket_polar[m0 + b] : in.static_polar[s0 + (b - M)]) != 0;
      const int area = cnt * w;                             // <= n_points * w <= 2^21
      if (lane == 0 && NR > 0) atomicAdd(&res[min(max(col, 0), NR - 1)], area);
      sum[4] += area;
      if (polar) sum[5] += area;
    }
  }
  if (lane == 0)
    for (int q = 0; q < 6; ++q) tot[wave][q] = sum[q];
  __syncthreads();                                          // the per-wave sums and every residue sum complete
  if (res_ok && out.res_buried) {
    int32_t* row = out.res_buried + in.res_off[g] + (long long)k * NR;
    for (int r = tid; r < NR; r += SA_THREADS) row[r] = bad ? 0 : res[r];
  }
  if (bad && lig_ok)
    for (int i = tid; i < NL; i += SA_THREADS) {
      if (out.lig_free) out.lig_free[lrow + i] = -1;
      if (out.lig_bound) out.lig_bound[lrow + i] = -1;
    }
  if (tid < 6 && out.totals) {
    long long v = 0;
    for (int w = 0; w < SA_WAVES; ++w) v += tot[w][tid];
    out.totals[6 * (size_t)f + tid] = bad ? -1 : v;
  }
}

// ------------------------------------------------------------------------------------------------ host
static int sa_err(const std::string& s) { return arg_err("dbfr_sasa", s); }

// the host copies of the index arrays, when the caller has them: every count, column, radius, weight and unit vector
static int sa_validate(const dbfr_sasa_in& d, const dbfr_sasa_in& h) {
  if (!h.frame_ptr || !h.lig_ptr || !h.lig_rad || !h.lig_w || !h.lig_polar || !h.pocket_ptr || !h.pocket_rad || !h.pocket_w ||
      !h.pocket_col || !h.pocket_polar || !h.res_ptr || !h.points ||
      (d.static_ptr && (!h.static_ptr || !h.static_rad || !h.static_w || !h.static_col || !h.static_polar)))
    return sa_err("host: a host copy of an index array is missing");
  const int G = d.n_group;
  const char* fn = "dbfr_sasa";
  if (const int rc = frame_ptr_err(fn, h.frame_ptr, G, d.n_frame)) return rc;
  for (int k = 0; k < d.n_points; ++k) {
    const double x = h.points[3 * k], y = h.points[3 * k + 1], z = h.points[3 * k + 2];
    if (!(std::fabs(std::sqrt(x * x + y * y + z * z) - 1.0) <= 1e-4)) return sa_err("point " + std::to_string(k) + " is no unit vector");
  }
  auto weight_ok = [&](int w) { return w > 0 && (long long)w * d.n_points <= SA_MAX_WN; };
  for (int g = 0; g < G; ++g) {
    const std::string where = "group " + std::to_string(g) + ": ";
    const int n0 = h.lig_ptr[g], NL = h.lig_ptr[g + 1] - n0, m0 = h.pocket_ptr[g], M = h.pocket_ptr[g + 1] - m0,
              s0 = d.static_ptr ? h.static_ptr[g] : 0, S = d.static_ptr ? h.static_ptr[g + 1] - s0 : 0, NR = h.res_ptr[g + 1] - h.res_ptr[g];
    if (const int rc = group_counts_err(fn, where, {{h.frame_ptr[g + 1] - h.frame_ptr[g]}, {NL, "ligand atoms", "max_lig", d.max_lig},
                                                    {M, "pocket atoms", "max_pocket", d.max_pocket}, {S},
                                                    {NR, "residue columns", "max_res", d.max_res}}))
      return rc;
    for (int i = 0; i < NL; ++i) {
      if (!(h.lig_rad[n0 + i] > 0.f && h.lig_rad[n0 + i] <= 4.f)) return sa_err(where + "the radius of ligand atom " + std::to_string(i) + " lies outside (0, 4]");
      if (!weight_ok(h.lig_w[n0 + i]))
        return sa_err(where + "the weight of ligand atom " + std::to_string(i) + " is not positive or n_points * weight exceeds 2^21");
    }
    auto weight_err = [&](int b) {
      return weight_ok(b < M ? h.pocket_w[m0 + b] : h.static_w[s0 + b - M]) ? DBFR_OK
          : sa_err(where + "the weight of receptor atom " + std::to_string(b) + " is not positive or n_points * weight exceeds 2^21");
    };
    if (const int rc = receptor_atoms_err(fn, where, M, S, h.pocket_rad + m0, d.static_ptr ? h.static_rad + s0 : nullptr, h.pocket_col + m0,
                                          d.static_ptr ? h.static_col + s0 : nullptr, NR, weight_err))
      return rc;
  }
  return DBFR_OK;
}

extern "C" int dbfr_sasa(const dbfr_sasa_in* in, const dbfr_sasa_opts* opts, const dbfr_sasa_out* out, void* hip_stream) {
  if (!in || !out) return sa_err("null argument");
  if (in->n_group < 0 || in->n_frame < 0) return sa_err("negative n_group / n_frame");
  if (in->max_lig < 0 || in->max_lig > SA_MAX_LIG) return limit_err("dbfr_sasa", "max_lig (ligand atoms)", in->max_lig, 0, SA_MAX_LIG);
  if (in->max_pocket < 0 || in->max_pocket > SA_MAX_POCKET) return limit_err("dbfr_sasa", "max_pocket (pocket atoms)", in->max_pocket, 0, SA_MAX_POCKET);
  if (in->max_res < 0 || in->max_res > SA_MAX_RES) return limit_err("dbfr_sasa", "max_res (residue columns)", in->max_res, 0, SA_MAX_RES);
  if (in->cand_cap != 0 && (in->cand_cap < SA_THREADS || in->cand_cap > SA_CAND_MAX))
    return limit_err("dbfr_sasa", "cand_cap (receptor atoms kept in LDS)", in->cand_cap, SA_THREADS, SA_CAND_MAX);
  if (in->n_points < 64 || in->n_points > SA_MAX_POINTS || in->n_points % 64 != 0)
    return sa_err("n_points " + std::to_string(in->n_points) + " must be a multiple of 64 in [64, 512]");
  dbfr_sasa_opts o = {1.4f};
  if (opts) o = *opts;
  if (!(o.probe >= 0.f && o.probe <= 2.f)) return sa_err("probe must lie in [0, 2] A and must not be NaN");
  if (in->n_frame == 0) return DBFR_OK;
  if (in->n_group == 0) return sa_err("frames without groups");
  if (!in->frame_ptr || !in->lig_ptr || !in->lig_pos_off || !in->lig_pos || !in->lig_rad || !in->lig_w || !in->lig_polar || !in->pocket_ptr ||
      !in->pocket_pos_off || !in->pocket_pos || !in->pocket_rad || !in->pocket_w || !in->pocket_col || !in->pocket_polar || !in->res_ptr ||
      !in->res_off || !in->points)
    return sa_err("frame_ptr / lig_ptr / lig_pos_off / lig_pos / lig_rad / lig_w / lig_polar / pocket_ptr / pocket_pos_off / pocket_pos / "
                  "pocket_rad / pocket_w / pocket_col / pocket_polar / res_ptr / res_off / points missing");
  if (in->static_ptr && (!in->static_pos || !in->static_rad || !in->static_w || !in->static_col || !in->static_polar))
    return sa_err("static_ptr given without static_pos / static_rad / static_w / static_col / static_polar");
  if (in->host) {
    const int rc = sa_validate(*in, *static_cast<const dbfr_sasa_in*>(in->host));
    if (rc != DBFR_OK) return rc;
  }
  SaArgs a;
  a.in = *in;
  a.in.host = nullptr;
  a.out = *out;
  a.probe = o.probe;
  a.cap = in->cand_cap ? in->cand_cap : SA_CAND;
  const size_t lds = 20 * (size_t)a.cap + 4 * (size_t)in->max_res + 16;
  HIPCHECK(launch_frames(k_sasa, in->n_frame, SA_THREADS, lds, hip_stream, a));
  return DBFR_OK;
}
