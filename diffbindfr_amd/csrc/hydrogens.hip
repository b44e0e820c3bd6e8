// Polar hydrogens and angle-checked hydrogen bonds of poses: the ligand's hydrogens and the pocket's polar hydrogens rebuilt
// from the heavy atoms of every frame of a ragged batch, the hydroxyl / thiol / ammonium rotors turned towards their
// acceptors, and the hydrogen bonds across the interface, in one launch.  include/dbfr.h states the definitions;
// docs/hydrogens.md the layout and the limits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/dbfr.h"
#include "common.h"
#include "frames.h"

// One workgroup per frame.  The ligand's heavy atoms (with their acceptor flag and neighbours) and its hydrogens live in LDS.
// Hydrogens that are no rotor are placed first, one per thread; the box of the ligand and of the pocket rotors' parents then
// rejects receptor atoms, and the receptor acceptors inside it are compacted in index order into an LDS list (when the list is
// too short every later loop reads the receptor from memory instead: the same expressions either way).  A wave takes a
// rotor: its K n_h candidate positions go to LDS, the lanes share the candidate acceptors and keep one minimum per k; the
// lowest k of the smallest minimum wins.  Bonds with a ligand donor: donors in order, the acceptor list in tiles of one
// acceptor per thread, compacted by ballot prefixes; bonds with a pocket donor: the pocket hydrogens (sorted by parent) in
// tiles, the first hydrogen of a parent walks the ligand's acceptors, counts, and a prefix sum of the counts gives its slots.
// Every reduction is a minimum with its index or an integer sum / or.
#define HY_THREADS FR_THREADS
#define HY_WAVES FR_WAVES
#define HY_MAX_LIG 256
#define HY_MAX_LH 256
#define HY_MAX_LROT 64
#define HY_MAX_RH 4096
#define HY_MAX_RES 16384
#define HY_MAX_BOND 64
#define HY_MAX_K 12
#define HY_MAX_NH 3
#define HY_CAND 2048               // receptor acceptors per frame kept in LDS (32 KB)
#define HY_MARGIN 0.01f            // A: the box filter is wider than the tests behind it by this much

struct HyArgs {
  dbfr_hydrogens_in in;
  dbfr_hydrogens_opts o;
  dbfr_hydrogens_out out;
  int cap;
  float cos_dha, cos_acc;
};

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 v3(float x, float y, float z) { return {x, y, z}; }
__device__ __forceinline__ V3 v3(const float* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ V3 v3(float4 p) { return {p.x, p.y, p.z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 unit(V3 a) {
  const float n = sqrtf(dot(a, a));
  return {a.x / n, a.y / n, a.z / n};
}
__device__ __forceinline__ float dist(V3 a, V3 b) { return sqrtf(dot(a - b, a - b)); }
// the cosine of the angle at `at` between the directions to u and to v
__device__ __forceinline__ float cos_at(V3 at, V3 u, V3 v) {
  const V3 a = u - at, b = v - at;
  return dot(a, b) / (sqrtf(dot(a, a)) * sqrtf(dot(b, b)));
}

// the hydrogen of one record (the definitions of include/dbfr.h); (c, s): the cosine and sine of the rotor's k steps
__device__ __forceinline__ V3 hy_place(int kind, V3 p, V3 q, V3 r, float4 f, float c, float s) {
  if (kind == 1) return p + f.x * unit(unit(p - q) + unit(p - r));
  const V3 e1 = kind == 0 ? unit(q - p) : unit(p - q);
  const V3 w = r - (kind == 0 ? p : q);
  const V3 e2 = unit(w - dot(w, e1) * e1);
  const V3 e3 = cross(e1, e2);
  float b2 = f.y, b3 = f.z;
  if (kind != 0) {
    b2 = f.y * (c * f.z - s * f.w);
    b3 = f.y * (s * f.z + c * f.w);
  }
  return p + f.x * e1 + b2 * e2 + b3 * e3;
}

// (c, s) of k steps: k complex products, every one rounded
__device__ __forceinline__ void hy_steps(int k, float cs, float ss, float& c, float& s) {
  c = 1.f; s = 0.f;
  for (int i = 0; i < k; ++i) {
    const float nc = c * cs - s * ss, ns = s * cs + c * ss;
    c = nc; s = ns;
  }
}

// the prefix sums of a workgroup's counts: slot = base + the counts of the threads before, total = all.  ONE barrier.
__device__ __forceinline__ void hy_block_scan(int c, int base, int* wcnt, int lane, int wave, int& slot, int& total) {
  int incl = c;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wcnt[wave] = incl;
  __syncthreads();
  int off = base, tot = 0;
  for (int w = 0; w < HY_WAVES; ++w) {
    off += w < wave ? wcnt[w] : 0;
    tot += wcnt[w];
  }
  slot = off + incl - c;
  total = tot;
}

__global__ __launch_bounds__(HY_THREADS) void k_hydrogens(HyArgs a) {
  __shared__ float4 lx[HY_MAX_LIG];                         // x, y, z, acceptor flag
  __shared__ int lnb[HY_MAX_LIG][3];
  __shared__ int ldon[HY_MAX_LIG];                          // the atom carries a hydrogen
  __shared__ float4 lh[HY_MAX_LH];                          // the ligand's hydrogens
  __shared__ int lhp[HY_MAX_LH];                            // parent + 65536 flags
  __shared__ int lhb[HY_MAX_LH];                            // 1: the hydrogen of a bond
  __shared__ float4 racc[HY_CAND];                          // x, y, z, receptor atom (bits) of the acceptors in the box
  __shared__ unsigned rbits[HY_MAX_RES / 16];               // 2 bits per residue column
  __shared__ float4 rpos[HY_WAVES][HY_MAX_K * HY_MAX_NH];   // a rotor's candidate positions
  __shared__ int wcnt[HY_WAVES];
  __shared__ float redf[HY_WAVES][8];
  const dbfr_hydrogens_in& in = a.in;
  const dbfr_hydrogens_out& out = a.out;
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = frame_group(in.frame_ptr, in.n_group, f);
  const int k = f - in.frame_ptr[g];
  const int KB = a.o.max_bond;
  const int l0 = in.lig_ptr[g], N = in.lig_ptr[g + 1] - l0;
  const int lh0 = in.lh_ptr[g], NHL = in.lh_ptr[g + 1] - lh0;
  const int lr0 = in.lrot_ptr[g], NRL = in.lrot_ptr[g + 1] - lr0;
  const int m0 = in.pocket_ptr[g], M = in.pocket_ptr[g + 1] - m0;
  const int s0 = in.static_ptr ? in.static_ptr[g] : 0, S = in.static_ptr ? in.static_ptr[g + 1] - s0 : 0;
  const int rh0 = in.rh_ptr[g], NHR = in.rh_ptr[g + 1] - rh0;
  const int rr0 = in.rrot_ptr[g], NRR = in.rrot_ptr[g + 1] - rr0;
  const int NR = in.res_ptr[g + 1] - in.res_ptr[g];
  bool bad = N < 1 || N > in.max_lig || N > HY_MAX_LIG || NHL < 0 || NHL > in.max_lig_h || NHL > HY_MAX_LH || NRL < 0 ||
             NRL > in.max_lig_rot || M < 0 || S < 0 || NHR < 0 || NHR > in.max_rec_h || NRR < 0 || NR < 0 || NR > in.max_res ||
             NR > HY_MAX_RES;
  const bool bad_counts = bad;
  const int MR = bad ? 0 : M + S;
  const Receptor rec = {in.pocket_pos + 3 * (in.pocket_pos_off[g] + (long long)k * M), in.static_pos + 3 * (size_t)s0, nullptr, nullptr, M};
  const int32_t* pmeta = in.pocket_meta + 4 * (size_t)m0;
  const int32_t* smeta = in.static_meta + 4 * (size_t)s0;
  const int32_t* lhi = in.lh_i + 8 * (size_t)lh0;
  const float4* lhf = reinterpret_cast<const float4*>(in.lh_f) + lh0;
  const int32_t* rhi = in.rh_i + 8 * (size_t)rh0;
  const float4* rhf = reinterpret_cast<const float4*>(in.rh_f) + rh0;
  float* olh = out.lig_h + 3 * (in.lh_out_off[g] + (long long)k * NHL);
  float* orh = out.rec_h + 3 * (in.rh_out_off[g] + (long long)k * NHR);
  int32_t* olk = out.lig_k + in.lk_off[g] + (long long)k * NRL;
  int32_t* ork = out.rec_k + in.rk_off[g] + (long long)k * NRR;
  uint8_t* ores = out.res_bits + in.res_off[g] + (long long)k * NR;
  int32_t* obi = out.bond_i + 4 * (size_t)f * KB;
  float* obf = out.bond_f + 3 * (size_t)f * KB;
  const float hb = a.o.hb_dist, hbh = a.o.hb_h_dist;
  int bad_atom = 0;
  FrameBox box;
  if (!bad) {
    const float* lp = in.lig_pos + 3 * (in.lig_pos_off[g] + (long long)k * N);
    for (int i = tid; i < N; i += HY_THREADS) {
      const float x = lp[3 * i], y = lp[3 * i + 1], z = lp[3 * i + 2];
      bad_atom |= !atom_ok(x, y, z);
      lx[i] = make_float4(x, y, z, in.lig_acc[l0 + i] ? 1.f : 0.f);
      for (int q = 0; q < 3; ++q) lnb[i][q] = in.lig_nbr[3 * (size_t)(l0 + i) + q];
      ldon[i] = 0;
      box.add(x, y, z, 0.f);
    }
    for (int b = tid; b < MR; b += HY_THREADS) {
      const float* y = rec.pos(b);
      bad_atom |= !atom_ok(y[0], y[1], y[2]);
    }
    for (int h = tid; h < NHL; h += HY_THREADS) lhb[h] = 0;
    for (int w = tid; w < (NR + 15) / 16; w += HY_THREADS) rbits[w] = 0u;
  }
  bad = __syncthreads_or(bad_atom) || bad;                  // uniform over the workgroup; the ligand complete in LDS
  if (bad) {                                                // counts outside the stated maxima or unusable atoms
    if (tid < 3) out.counts[3 * (size_t)f + tid] = -1;
    if (tid == 0) out.n_bond[f] = -1;
    for (int e = tid; e < KB; e += HY_THREADS) {
      for (int q = 0; q < 4; ++q) obi[4 * e + q] = -1;
      for (int q = 0; q < 3; ++q) obf[3 * e + q] = NAN;
    }
    if (!bad_counts) {                                      // the rows of a frame whose counts are wrong are not known
      for (int t = tid; t < 3 * NHL; t += HY_THREADS) olh[t] = 0.f;
      for (int t = tid; t < 3 * NHR; t += HY_THREADS) orh[t] = 0.f;
      for (int t = tid; t < NRL; t += HY_THREADS) olk[t] = 0;
      for (int t = tid; t < NRR; t += HY_THREADS) ork[t] = 0;
      for (int t = tid; t < NR; t += HY_THREADS) ores[t] = 0;
    }
    return;
  }
  // the hydrogens that are no rotor's, and the box of the ligand with the pocket rotors' parents
  for (int h = tid; h < NHL; h += HY_THREADS) {
    const int32_t* r = lhi + 8 * (size_t)h;
    lhp[h] = r[0] | (r[5] & 1) << 16;
    ldon[r[0]] = 1;                                         // (the same value from every writer)
    if (r[4] < 0) {
      const V3 H = hy_place(r[3], v3(lx[r[0]]), v3(lx[r[1]]), v3(lx[r[2]]), lhf[h], 1.f, 0.f);
      lh[h] = make_float4(H.x, H.y, H.z, 0.f);
      olh[3 * h] = H.x; olh[3 * h + 1] = H.y; olh[3 * h + 2] = H.z;
    }
  }
  for (int h = tid; h < NHR; h += HY_THREADS) {
    const int32_t* r = rhi + 8 * (size_t)h;
    const V3 P = v3(rec.pos(r[0]));
    if (r[4] < 0) {
      const V3 H = hy_place(r[3], P, v3(rec.pos(r[1])), v3(rec.pos(r[2])), rhf[h], 1.f, 0.f);
      orh[3 * (size_t)h] = H.x; orh[3 * (size_t)h + 1] = H.y; orh[3 * (size_t)h + 2] = H.z;
    } else {
      box.add(P.x, P.y, P.z, 0.f);
    }
  }
  box.block_reduce(redf, lane, wave);                       // (its barrier: lh, lhp and ldon complete)
  // the receptor acceptors in the box, in index order
  const float grow = hb + HY_MARGIN;
  int nacc = 0;                                             // uniform
  for (int b0 = 0; b0 < MR; b0 += HY_THREADS) {
    const int b = b0 + tid;
    bool c = false;
    float x = 0.f, y = 0.f, z = 0.f;
    if (b < MR && (rec.sel(b, pmeta, smeta, 4)[0] & 1)) {
      const float* p = rec.pos(b);
      x = p[0]; y = p[1]; z = p[2];
      c = box.touches(x, y, z, grow);
    }
    int slot, tot;
    block_compact(c, nacc, wcnt, lane, wave, slot, tot);
    if (c && slot < a.cap) racc[slot] = make_float4(x, y, z, __int_as_float(b));   // a full list drops the entry: `spill` below
    nacc += tot;
    __syncthreads();                                        // wcnt is rewritten by the next tile
  }
  const bool spill = nacc > a.cap;                          // uniform: the loops below read every receptor atom instead
  const int ncand = spill ? MR : nacc;
  // candidate j: the acceptor's position and receptor atom; false when receptor atom j is no acceptor (spill only)
  auto cand = [&](int j, V3& A, int& b) -> bool {
    if (!spill) {
      const float4 e = racc[j];
      A = v3(e);
      b = __float_as_int(e.w);
      return true;
    }
    b = j;
    if (!(rec.sel(j, pmeta, smeta, 4)[0] & 1)) return false;
    A = v3(rec.pos(j));
    return true;
  };
  // rotors: one per wave
  const int NROT = NRL + NRR;
  for (int ro0 = 0; ro0 < NROT; ro0 += HY_WAVES) {
    const int ro = ro0 + wave;
    const bool live = ro < NROT, lig = ro < NRL;
    int h0 = 0, nh = 1, K = 1, own = -1;
    float cs = 1.f, ss = 0.f;
    V3 P = v3(0.f, 0.f, 0.f), Q = P, R = P;
    int kind = 3;
    if (live) {
      const int32_t* ri = lig ? in.lrot_i + 4 * (size_t)(lr0 + ro) : in.rrot_i + 4 * (size_t)(rr0 + ro - NRL);
      const float* rf = lig ? in.lrot_f + 2 * (size_t)(lr0 + ro) : in.rrot_f + 2 * (size_t)(rr0 + ro - NRL);
      h0 = ri[0]; nh = ri[1]; K = ri[2];
      cs = rf[0]; ss = rf[1];
      const int32_t* r = (lig ? lhi : rhi) + 8 * (size_t)h0;
      kind = r[3];
      if (lig) {
        P = v3(lx[r[0]]); Q = v3(lx[r[1]]); R = v3(lx[r[2]]);
      } else {
        P = v3(rec.pos(r[0])); Q = v3(rec.pos(r[1])); R = v3(rec.pos(r[2]));
        own = pmeta[4 * (size_t)r[0]] >> 8;
      }
      if (lane < K * nh) {
        const int kk = lane / nh, j = lane - kk * nh;
        float c, s;
        hy_steps(kk, cs, ss, c, s);
        const V3 H = hy_place(kind, P, Q, R, (lig ? lhf : rhf)[h0 + j], c, s);
        rpos[wave][lane] = make_float4(H.x, H.y, H.z, 0.f);
      }
    }
    __syncthreads();                                        // the candidate positions complete
    float best[HY_MAX_K];
#pragma unroll
    for (int kk = 0; kk < HY_MAX_K; ++kk) best[kk] = INFINITY;
    if (live) {
      for (int j = lane; j < ncand; j += 64) {
        V3 A;
        int b;
        if (!cand(j, A, b)) continue;
        if (!lig && (rec.sel(b, pmeta, smeta, 4)[0] >> 8) == own) continue;
        if (!(dist(P, A) <= hb)) continue;
#pragma unroll
        for (int kk = 0; kk < HY_MAX_K; ++kk)
          if (kk < K)
            for (int j2 = 0; j2 < nh; ++j2) best[kk] = fminf(best[kk], dist(v3(rpos[wave][kk * nh + j2]), A));
      }
      if (!lig)
        for (int i = lane; i < N; i += 64) {
          const float4 q = lx[i];
          if (q.w == 0.f || !(dist(P, v3(q)) <= hb)) continue;
#pragma unroll
          for (int kk = 0; kk < HY_MAX_K; ++kk)
            if (kk < K)
              for (int j2 = 0; j2 < nh; ++j2) best[kk] = fminf(best[kk], dist(v3(rpos[wave][kk * nh + j2]), v3(q)));
        }
    }
    float bv = INFINITY;
    int bk = 0;
#pragma unroll
    for (int kk = 0; kk < HY_MAX_K; ++kk) {
      const float v = wave_min(best[kk]);
      if (kk < K && v < bv) { bv = v; bk = kk; }           // the lowest k on a tie
    }
    if (live) {
      if (lane < nh) {
        const float4 H = rpos[wave][bk * nh + lane];
        const int h = h0 + lane;
        if (lig) {
          lh[h] = H;
          olh[3 * h] = H.x; olh[3 * h + 1] = H.y; olh[3 * h + 2] = H.z;
        } else {
          orh[3 * (size_t)h] = H.x; orh[3 * (size_t)h + 1] = H.y; orh[3 * (size_t)h + 2] = H.z;
        }
      }
      if (lane == 0) (lig ? olk : ork)[lig ? ro : ro - NRL] = bk;
    }
    __syncthreads();                                        // rpos is rewritten by the next rotor; lh and rec_h complete at the end
  }
  // bonds with a ligand donor, in (D, A) order
  int nb = 0;                                               // uniform
  for (int D = 0; D < N; ++D) {
    if (!ldon[D]) continue;
    const V3 Dp = v3(lx[D]);
    for (int j0 = 0; j0 < ncand; j0 += HY_THREADS) {
      const int j = j0 + tid;
      V3 A = Dp;
      int b = 0, bh = -1;
      float bd = INFINITY, bc = 0.f, dDA = 0.f;
      if (j < ncand && cand(j, A, b) && (dDA = dist(Dp, A)) <= hb) {
        const int32_t* mt = rec.sel(b, pmeta, smeta, 4);
        for (int h = 0; h < NHL; ++h) {
          if ((lhp[h] & 0xffff) != D) continue;
          const V3 H = v3(lh[h]);
          const float dHA = dist(H, A);
          if (!(dHA <= hbh)) continue;
          const float c = cos_at(H, Dp, A);
          if (!(c <= a.cos_dha)) continue;
          bool ok = true;
          for (int q = 1; q < 4; ++q)
            if (mt[q] >= 0) ok = ok && cos_at(A, v3(rec.pos(mt[q])), H) <= a.cos_acc;
          if (ok && dHA < bd) { bd = dHA; bh = h; bc = c; }
        }
      }
      const bool hit = bh >= 0;
      int slot, tot;
      block_compact(hit, nb, wcnt, lane, wave, slot, tot);
      if (hit) {
        lhb[bh] = 1;
        const int col = rec.sel(b, pmeta, smeta, 4)[0] >> 8;
        atomicOr(&rbits[col >> 4], 2u << 2 * (col & 15));
        if (slot < KB) {
          obi[4 * slot] = 0; obi[4 * slot + 1] = D; obi[4 * slot + 2] = bh; obi[4 * slot + 3] = b;
          obf[3 * slot] = dDA; obf[3 * slot + 1] = bd; obf[3 * slot + 2] = bc;
        }
      }
      nb += tot;
      __syncthreads();                                      // wcnt is rewritten by the next tile
    }
  }
  const int n_don = nb;
  // bonds with a pocket donor: the first hydrogen of a parent takes the parent's bonds
  for (int hb0 = 0; hb0 < NHR; hb0 += HY_THREADS) {
    const int h = hb0 + tid;
    int D = -1, hend = h;
    V3 Dp = v3(0.f, 0.f, 0.f);
    if (h < NHR) {
      D = rhi[8 * (size_t)h];
      if (h > 0 && rhi[8 * (size_t)(h - 1)] == D) D = -1;   // not the first of its parent
    }
    if (D >= 0) {
      Dp = v3(rec.pos(D));
      if (!box.touches(Dp.x, Dp.y, Dp.z, grow)) D = -1;
      for (hend = h + 1; hend < NHR && rhi[8 * (size_t)hend] == rhi[8 * (size_t)h]; ++hend) {}
    }
    int cnt = 0, slot = 0, tot = 0;
    for (int pass = 0; pass < 2; ++pass) {
      if (D >= 0 && (pass == 0 || cnt > 0))
        for (int i = 0; i < N; ++i) {
          const float4 q = lx[i];
          if (q.w == 0.f) continue;
          const V3 A = v3(q);
          const float dDA = dist(Dp, A);
          if (!(dDA <= hb)) continue;
          int bh = -1;
          float bd = INFINITY, bc = 0.f;
          for (int hh = h; hh < hend; ++hh) {
            const V3 H = v3(orh + 3 * (size_t)hh);
            const float dHA = dist(H, A);
            if (!(dHA <= hbh)) continue;
            const float c = cos_at(H, Dp, A);
            if (!(c <= a.cos_dha)) continue;
            bool ok = true;
            for (int q2 = 0; q2 < 3; ++q2)
              if (lnb[i][q2] >= 0) ok = ok && cos_at(A, v3(lx[lnb[i][q2]]), H) <= a.cos_acc;
            if (ok && dHA < bd) { bd = dHA; bh = hh; bc = c; }
          }
          if (bh < 0) continue;
          if (pass == 0) {
            ++cnt;
          } else {
            if (slot < KB) {
              obi[4 * slot] = 1; obi[4 * slot + 1] = D; obi[4 * slot + 2] = bh; obi[4 * slot + 3] = i;
              obf[3 * slot] = dDA; obf[3 * slot + 1] = bd; obf[3 * slot + 2] = bc;
            }
            ++slot;
          }
        }
      if (pass == 0) {
        hy_block_scan(cnt, nb, wcnt, lane, wave, slot, tot);
        if (cnt > 0) {
          const int col = pmeta[4 * (size_t)D] >> 8;
          atomicOr(&rbits[col >> 4], 1u << 2 * (col & 15));
        }
      }
    }
    nb += tot;
    __syncthreads();                                        // wcnt is rewritten by the next tile
  }
  __syncthreads();                                          // lhb and rbits complete
  for (int e = min(nb, KB) + tid; e < KB; e += HY_THREADS) {                  // the slots not used
    for (int q = 0; q < 4; ++q) obi[4 * e + q] = -1;
    for (int q = 0; q < 3; ++q) obf[3 * e + q] = NAN;
  }
  for (int c = tid; c < NR; c += HY_THREADS) ores[c] = (uint8_t)(rbits[c >> 4] >> 2 * (c & 15) & 3u);
  int unsat = 0;
  for (int h = tid; h < NHL; h += HY_THREADS) unsat += (lhp[h] >> 16 & 1) && !lhb[h];
  unsat = wave_sum(unsat);
  if (lane == 0) wcnt[wave] = unsat;
  __syncthreads();
  if (tid == 0) {
    int u = 0;
    for (int w = 0; w < HY_WAVES; ++w) u += wcnt[w];
    out.counts[3 * (size_t)f] = n_don;
    out.counts[3 * (size_t)f + 1] = nb - n_don;
    out.counts[3 * (size_t)f + 2] = u;
    out.n_bond[f] = nb;
  }
}

// ------------------------------------------------------------------------------------------------ host
static const char* HY_FN = "dbfr_hydrogens";

// the hydrogens and rotors of one side of one group: n_atom = the atoms q and r may name, n_parent those p may name
static int hy_side_err(const std::string& where, const char* side, const int32_t* hi, int NH, const int32_t* ri, const float* rf, int NROT,
                       int n_atom, int n_parent, bool sorted) {
  for (int h = 0; h < NH; ++h) {
    const int32_t* r = hi + 8 * (size_t)h;
    const std::string who = where + side + " hydrogen " + std::to_string(h);
    if (r[0] < 0 || r[0] >= n_parent || r[1] < 0 || r[1] >= n_atom || r[2] < 0 || r[2] >= n_atom)
      return arg_err(HY_FN, who + " names an atom outside the group");
    if (r[0] == r[1] || r[0] == r[2] || r[1] == r[2]) return arg_err(HY_FN, who + " names an atom twice");
    if (r[3] < 0 || r[3] > 3) return arg_err(HY_FN, who + ": the kind is not 0, 1, 2 or 3");
    if (r[4] < -1 || r[4] >= NROT || (r[4] >= 0) != (r[3] == 3)) return arg_err(HY_FN, who + ": the rotor is out of range or does not fit the kind");
    if (sorted && h > 0 && r[0] < hi[8 * (size_t)(h - 1)]) return arg_err(HY_FN, who + ": the hydrogens are not sorted by parent");
  }
  for (int j = 0; j < NROT; ++j) {
    const int32_t* r = ri + 4 * (size_t)j;
    const std::string who = where + side + " rotor " + std::to_string(j);
    if (r[1] < 1 || r[1] > HY_MAX_NH || r[2] < 1 || r[2] > HY_MAX_K) return arg_err(HY_FN, who + ": 1 to 3 hydrogens and 1 to 12 steps");
    if (r[0] < 0 || r[0] > NH - r[1]) return arg_err(HY_FN, who + " names a hydrogen outside the group");
    for (int q = 0; q < r[1]; ++q) {
      const int32_t* h = hi + 8 * (size_t)(r[0] + q);
      if (h[4] != j || h[0] != hi[8 * (size_t)r[0]] || h[1] != hi[8 * (size_t)r[0] + 1] || h[2] != hi[8 * (size_t)r[0] + 2])
        return arg_err(HY_FN, who + ": its hydrogens do not name it or differ in their atoms");
    }
    if (std::isnan(rf[2 * (size_t)j]) || std::isnan(rf[2 * (size_t)j + 1])) return arg_err(HY_FN, who + ": the step is NaN");
  }
  return DBFR_OK;
}

// the host copies of the index arrays, when the caller has them
static int hy_validate(const dbfr_hydrogens_in& d, const dbfr_hydrogens_in& h) {
  if (!h.frame_ptr || !h.lig_ptr || !h.lig_acc || !h.lig_nbr || !h.lh_ptr || !h.lh_i || !h.lh_f || !h.lrot_ptr || !h.lrot_i || !h.lrot_f ||
      !h.pocket_ptr || !h.pocket_meta || !h.rh_ptr || !h.rh_i || !h.rh_f || !h.rrot_ptr || !h.rrot_i || !h.rrot_f || !h.res_ptr ||
      (d.static_ptr && (!h.static_ptr || !h.static_meta)))
    return arg_err(HY_FN, "host: a host copy of an index array is missing");
  const int G = d.n_group;
  if (const int rc = frame_ptr_err(HY_FN, h.frame_ptr, G, d.n_frame)) return rc;
  for (int g = 0; g < G; ++g) {
    const std::string where = "group " + std::to_string(g) + ": ";
    const int n0 = h.lig_ptr[g], N = h.lig_ptr[g + 1] - n0, lh0 = h.lh_ptr[g], NHL = h.lh_ptr[g + 1] - lh0, lr0 = h.lrot_ptr[g],
              NRL = h.lrot_ptr[g + 1] - lr0, m0 = h.pocket_ptr[g], M = h.pocket_ptr[g + 1] - m0, s0 = d.static_ptr ? h.static_ptr[g] : 0,
              S = d.static_ptr ? h.static_ptr[g + 1] - s0 : 0, rh0 = h.rh_ptr[g], NHR = h.rh_ptr[g + 1] - rh0, rr0 = h.rrot_ptr[g],
              NRR = h.rrot_ptr[g + 1] - rr0, NR = h.res_ptr[g + 1] - h.res_ptr[g];
    if (const int rc = group_counts_err(HY_FN, where, {{h.frame_ptr[g + 1] - h.frame_ptr[g]}, {N, "ligand atoms", "max_lig", d.max_lig},
                                                       {NHL, "ligand hydrogens", "max_lig_h", d.max_lig_h},
                                                       {NRL, "ligand rotors", "max_lig_rot", d.max_lig_rot}, {M}, {S},
                                                       {NHR, "pocket hydrogens", "max_rec_h", d.max_rec_h}, {NRR},
                                                       {NR, "residue columns", "max_res", d.max_res}}))
      return rc;
    if (N < 1) return arg_err(HY_FN, where + "no ligand atoms");
    for (int i = 0; i < 3 * N; ++i)
      if (h.lig_nbr[3 * (size_t)n0 + i] < -1 || h.lig_nbr[3 * (size_t)n0 + i] >= N)
        return arg_err(HY_FN, where + "a neighbour of ligand atom " + std::to_string(i / 3) + " lies outside the ligand");
    for (int b = 0; b < M + S; ++b) {
      const int32_t* mt = b < M ? h.pocket_meta + 4 * (size_t)(m0 + b) : h.static_meta + 4 * (size_t)(s0 + b - M);
      if (mt[0] < 0 || (mt[0] >> 8) >= NR) return arg_err(HY_FN, where + "the residue column of receptor atom " + std::to_string(b) + " is out of range");
      for (int q = 1; q < 4; ++q)
        if (mt[q] < -1 || mt[q] >= M + S) return arg_err(HY_FN, where + "a neighbour of receptor atom " + std::to_string(b) + " lies outside the receptor");
    }
    if (const int rc = hy_side_err(where, "ligand", h.lh_i + 8 * (size_t)lh0, NHL, h.lrot_i + 4 * (size_t)lr0, h.lrot_f + 2 * (size_t)lr0, NRL, N, N, false))
      return rc;
    if (const int rc = hy_side_err(where, "pocket", h.rh_i + 8 * (size_t)rh0, NHR, h.rrot_i + 4 * (size_t)rr0, h.rrot_f + 2 * (size_t)rr0, NRR, M + S, M, true))
      return rc;
  }
  return DBFR_OK;
}

extern "C" int dbfr_hydrogens(const dbfr_hydrogens_in* in, const dbfr_hydrogens_opts* opts, const dbfr_hydrogens_out* out, void* hip_stream) {
  const char* fn = HY_FN;
  if (!in || !out) return arg_err(fn, "null argument");
  if (in->n_group < 0 || in->n_frame < 0) return arg_err(fn, "negative n_group / n_frame");
  if (in->max_lig < 0 || in->max_lig > HY_MAX_LIG) return limit_err(fn, "max_lig (ligand heavy atoms)", in->max_lig, 0, HY_MAX_LIG);
  if (in->max_lig_h < 0 || in->max_lig_h > HY_MAX_LH) return limit_err(fn, "max_lig_h (ligand hydrogens)", in->max_lig_h, 0, HY_MAX_LH);
  if (in->max_lig_rot < 0 || in->max_lig_rot > HY_MAX_LROT) return limit_err(fn, "max_lig_rot (ligand rotors)", in->max_lig_rot, 0, HY_MAX_LROT);
  if (in->max_rec_h < 0 || in->max_rec_h > HY_MAX_RH) return limit_err(fn, "max_rec_h (pocket hydrogen records)", in->max_rec_h, 0, HY_MAX_RH);
  if (in->max_res < 0 || in->max_res > HY_MAX_RES) return limit_err(fn, "max_res (residue columns)", in->max_res, 0, HY_MAX_RES);
  if (in->cand_cap < 0 || in->cand_cap > HY_CAND) return limit_err(fn, "cand_cap (LDS acceptors)", in->cand_cap, 0, HY_CAND);
  dbfr_hydrogens_opts o = {3.5f, 2.5f, 120.f, 90.f, HY_MAX_BOND};
  if (opts) o = *opts;
  if (o.max_bond < 1 || o.max_bond > HY_MAX_BOND) return limit_err(fn, "max_bond (bonds kept per frame)", o.max_bond, 1, HY_MAX_BOND);
  if (!(o.hb_dist > 0.f && o.hb_dist <= 8.f)) return arg_err(fn, "hb_dist must lie in (0, 8] A");
  if (!(o.hb_h_dist >= 0.f && o.hb_h_dist <= 100.f)) return arg_err(fn, "hb_h_dist must lie in [0, 100] A");
  if (!(o.hb_dha_angle >= 0.f && o.hb_dha_angle <= 180.f) || !(o.hb_acc_angle >= 0.f && o.hb_acc_angle <= 180.f))
    return arg_err(fn, "hb_dha_angle and hb_acc_angle must lie in [0, 180] degrees");
  if (in->n_frame == 0) return DBFR_OK;
  if (in->n_group == 0) return arg_err(fn, "frames without groups");
  if (!in->frame_ptr || !in->lig_ptr || !in->lig_pos_off || !in->lig_pos || !in->lig_acc || !in->lig_nbr || !in->lh_ptr || !in->lh_i || !in->lh_f ||
      !in->lrot_ptr || !in->lrot_i || !in->lrot_f || !in->lh_out_off || !in->lk_off || !in->pocket_ptr || !in->pocket_pos_off || !in->pocket_pos ||
      !in->pocket_meta || !in->rh_ptr || !in->rh_i || !in->rh_f || !in->rrot_ptr || !in->rrot_i || !in->rrot_f || !in->rh_out_off || !in->rk_off ||
      !in->res_ptr || !in->res_off)
    return arg_err(fn, "an input array is missing (only static_ptr / static_pos / static_meta may be NULL)");
  if (in->static_ptr && (!in->static_pos || !in->static_meta)) return arg_err(fn, "static_ptr given without static_pos / static_meta");
  if (!out->lig_h || !out->rec_h || !out->lig_k || !out->rec_k || !out->counts || !out->n_bond || !out->bond_i || !out->bond_f || !out->res_bits)
    return arg_err(fn, "an output array is missing");
  if (in->host) {
    const int rc = hy_validate(*in, *static_cast<const dbfr_hydrogens_in*>(in->host));
    if (rc != DBFR_OK) return rc;
  }
  HyArgs a;
  a.in = *in;
  a.in.host = nullptr;
  a.o = o;
  a.out = *out;
  a.cap = in->cand_cap ? in->cand_cap : HY_CAND;
  a.cos_dha = (float)std::cos((double)o.hb_dha_angle * M_PI / 180.0);
  a.cos_acc = (float)std::cos((double)o.hb_acc_angle * M_PI / 180.0);
  HIPCHECK(launch_frames(k_hydrogens, in->n_frame, HY_THREADS, 0, hip_stream, a));
  return DBFR_OK;
}
