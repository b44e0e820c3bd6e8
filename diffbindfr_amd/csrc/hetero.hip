// Checks of poses against cofactors, metal ions and waters: per class the closest approach, the clash count and the lattice
// volume overlap, and per hetero atom the events (clash, displaced water, metal coordination, water bridge) of every frame of
// a ragged batch, in one launch.  include/dbfr.h states the definitions; docs/hetero.md the layout and the limits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/dbfr.h"
#include "common.h"
#include "frames.h"

// One workgroup per frame.  The ligand (positions, vdW and covalent radii, flag bits) is staged in LDS.  The hetero atoms of
// the group go past in tiles of one atom per thread: a thread walks the ligand once and has d_h, a_h, rho_h, the clash count,
// n_coord_h and p_h of its atom.  The waters of the tile that a polar ligand atom reaches are compacted into an LDS list with
// their bounding box; when there are any, the receptor (pocket atoms of the frame, then the static atoms of the group) streams
// past, one atom per thread, the polar atoms inside the box walk the list and the nearest one per water is the minimum of a
// packed 64-bit key (float bits of the distance, then the index: the order of non-negative floats is the order of their bits)
// taken with an LDS integer atomic.  The events of the tile are then compacted in index order, and so are the hetero atoms
// that can share a lattice point with the ligand.  The lattice passes, one per distinct scale, walk every ligand atom's box as
// posecheck.hip does and test an owned point against those candidates -- or, when the list was too short, against every hetero
// atom in memory: the same expression either way.  Every reduction is a min / max or an integer sum: the bits of a frame do
// not depend on the launch it is part of nor on the length of the list.
#define HC_THREADS FR_THREADS
#define HC_WAVES FR_WAVES
#define HC_MAX_LIG 256
#define HC_MAX_POCKET 8192
#define HC_MAX_RES 16384
#define HC_MAX_EVENT 256
#define HC_CAND 1024               // lattice candidates per frame kept in LDS (20 KB)
#define HC_MARGIN 0.01f            // A: candidate / neighbour / box filters are wider than the tests behind them by this much
#define HC_NO_KEY 0xffffffffffffffffull
#define HC_EMPTY_KEY 0x7f800000ffffffffull      // +inf, -1

struct HcArgs {
  dbfr_hetero_check_in in;
  dbfr_hetero_check_opts o;
  dbfr_hetero_check_out out;
  int cap;
};

__device__ __forceinline__ float hc_dist2(float px, float py, float pz, float qx, float qy, float qz) {
  const float dx = px - qx, dy = py - qy, dz = pz - qz;
  return dx * dx + dy * dy + dz * dz;
}

__device__ __forceinline__ unsigned long long hc_key(float v, int idx) {
  return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)idx;
}

__device__ __forceinline__ unsigned long long hc_min(unsigned long long p, unsigned long long q) { return q < p ? q : p; }

__device__ __forceinline__ unsigned long long hc_wave_min(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
    v = hc_min(v, ((unsigned long long)hi << 32) | lo);
  }
  return v;
}

__device__ __forceinline__ bool hc_radius_ok(float r) { return r > 0.f && r <= 4.f; }

__global__ __launch_bounds__(HC_THREADS) void k_hetero_check(HcArgs a) {
  __shared__ float4 lx[HC_MAX_LIG];                         // x, y, z, vdW radius
  __shared__ float lcov[HC_MAX_LIG];
  __shared__ int lflag[HC_MAX_LIG];
  __shared__ unsigned long long nbm[HC_MAX_LIG][4];         // bit c of atom a: c < a and their lattice spheres can meet
  __shared__ float4 cand[HC_CAND];                          // x, y, z, (vol_scale r)^2 of the lattice candidates
  __shared__ int ccls[HC_CAND];                             // their classes
  __shared__ float4 wat[HC_THREADS];                        // the tile's waters a polar ligand atom reaches
  __shared__ unsigned long long wkey[HC_THREADS];           // the nearest polar receptor atom of each
  __shared__ int wcnt[HC_WAVES];
  __shared__ float redf[HC_WAVES][8];
  __shared__ unsigned long long redk[HC_WAVES][3];
  __shared__ int redi[HC_WAVES][12];
  const dbfr_hetero_check_in& in = a.in;
  const dbfr_hetero_check_opts& o = a.o;
  const dbfr_hetero_check_out& out = a.out;
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = frame_group(in.frame_ptr, in.n_group, f);
  const int k = f - in.frame_ptr[g];
  const int K = o.max_event;
  const int l0 = in.lig_ptr[g], N = in.lig_ptr[g + 1] - l0;
  const int h0g = in.het_ptr[g], H = in.het_ptr[g + 1] - h0g;
  const int m0 = in.pocket_ptr[g], M = in.pocket_ptr[g + 1] - m0;
  const int s0 = in.static_ptr ? in.static_ptr[g] : 0, S = in.static_ptr ? in.static_ptr[g + 1] - s0 : 0;
  bool bad = N < 1 || N > in.max_lig || N > HC_MAX_LIG || H < 0 || M < 0 || M > in.max_pocket || S < 0;
  const int MR = bad ? 0 : M + S;
  const Receptor rec = {in.pocket_pos + 3 * (in.pocket_pos_off[g] + (long long)k * M), in.static_pos + 3 * (size_t)s0, nullptr, nullptr, M};
  const float* hp = in.het_pos + 3 * (size_t)h0g;
  const float* hrad = in.het_rad + h0g;
  const float* hcov = in.het_cov + h0g;
  const uint8_t* hcls = in.het_class + h0g;
  const uint8_t* hmet = in.het_metal + h0g;
  const uint8_t* ppol = in.pocket_polar + m0;
  const uint8_t* spol = in.static_polar + s0;
  const float vs0 = o.vol_scale[0], vs1 = o.vol_scale[1], vs2 = o.vol_scale[2], hg = o.grid;
  int bad_atom = 0;
  if (!bad) {
    const float* lp = in.lig_pos + 3 * (in.lig_pos_off[g] + (long long)k * N);
    for (int i = tid; i < N; i += HC_THREADS) {
      const float x = lp[3 * i], y = lp[3 * i + 1], z = lp[3 * i + 2], r = in.lig_rad[l0 + i], rc = in.lig_cov[l0 + i];
      bad_atom |= !atom_ok(x, y, z, r) || !hc_radius_ok(rc);
      lx[i] = make_float4(x, y, z, r);
      lcov[i] = rc;
      lflag[i] = in.lig_flags[l0 + i];
    }
    for (int h = tid; h < H; h += HC_THREADS)
      bad_atom |= !atom_ok(hp[3 * (size_t)h], hp[3 * (size_t)h + 1], hp[3 * (size_t)h + 2], hrad[h]) || !hc_radius_ok(hcov[h]) || hcls[h] > 2;
    for (int b = tid; b < MR; b += HC_THREADS) {
      const float* y = rec.pos(b);
      bad_atom |= !atom_ok(y[0], y[1], y[2]);
    }
  }
  bad = __syncthreads_or(bad_atom) || bad;                  // uniform over the workgroup; the ligand complete in LDS
  if (bad) {                                                // counts outside the stated maxima or unusable atoms: NaN / -1
    if (tid < 3) {
      const size_t q = 3 * (size_t)f + tid;
      if (out.min_dist) out.min_dist[q] = NAN;
      if (out.min_ratio) out.min_ratio[q] = NAN;
      if (out.worst) out.worst[q] = -1;
      if (out.n_clash) out.n_clash[q] = -1;
      if (out.vol_lig) out.vol_lig[q] = -1;
      if (out.vol_overlap) out.vol_overlap[q] = -1;
    }
    if (tid == 0) {
      if (out.n_displaced) out.n_displaced[f] = -1;
      if (out.n_bridge) out.n_bridge[f] = -1;
      if (out.n_coord) out.n_coord[f] = -1;
      if (out.passed) out.passed[f] = 0;
      if (out.n_event) out.n_event[f] = -1;
    }
    if (tid < K) {
      const size_t e = (size_t)f * K + tid;
      if (out.event_i)
        for (int q = 0; q < 6; ++q) out.event_i[6 * e + q] = -1;
      if (out.event_f)
        for (int q = 0; q < 3; ++q) out.event_f[3 * e + q] = NAN;
    }
    return;
  }
  // hetero pass: distances, ratios, clashes, events, lattice candidates
  float md0 = INFINITY, md1 = INFINITY, md2 = INFINITY;
  unsigned long long key0 = HC_EMPTY_KEY, key1 = HC_EMPTY_KEY, key2 = HC_EMPTY_KEY;
  int ncl0 = 0, ncl1 = 0, ncl2 = 0, ndis = 0, nbr = 0, nco = 0;
  int nev = 0, ncand = 0;                                   // uniform
  for (int hb = 0; hb < H; hb += HC_THREADS) {
    const int h = hb + tid;
    const bool live = h < H;
    float hx = 0.f, hy = 0.f, hz = 0.f, hr = 1.f, hc = 1.f;
    int cls = 0, metal = 0;
    if (live) {
      hx = hp[3 * (size_t)h]; hy = hp[3 * (size_t)h + 1]; hz = hp[3 * (size_t)h + 2];
      hr = hrad[h]; hc = hcov[h];
      cls = hcls[h]; metal = hmet[h] != 0;
    }
    const float vsc = cls == 0 ? vs0 : (cls == 1 ? vs1 : vs2), Rh = vsc * hr;
    float dmin = INFINITY, rho = INFINITY, pd = INFINITY;
    int amin = 0, ncl = 0, ncoord = 0, pa = -1;
    bool lc = false;
    if (live)
      for (int i = 0; i < N; ++i) {
        const float4 q = lx[i];
        const int fl = lflag[i];
        const float d = sqrtf(hc_dist2(q.x, q.y, q.z, hx, hy, hz));
        const float R = cls == 1 ? lcov[i] + hc : q.w + hr;
        const float ratio = d / R;
        if (d < dmin) { dmin = d; amin = i; }
        rho = fminf(rho, ratio);
        ncl += ratio < o.clash_ratio;
        ncoord += (fl & 2) && d <= o.metal_dist;
        if ((fl & 1) && d <= o.hbond_dist && d < pd) { pd = d; pa = i; }
        lc = lc || d < vsc * q.w + Rh + HC_MARGIN;
      }
    if (live) {
      const unsigned long long kh = hc_key(rho, h);
      if (cls == 0) { md0 = fminf(md0, dmin); key0 = hc_min(key0, kh); ncl0 += ncl; }
      else if (cls == 1) { md1 = fminf(md1, dmin); key1 = hc_min(key1, kh); ncl1 += ncl; }
      else { md2 = fminf(md2, dmin); key2 = hc_min(key2, kh); ncl2 += ncl; }
    }
    const bool clash = live && rho < o.clash_ratio;
    const bool displaced = live && cls == 2 && dmin < o.displace_dist;
    const bool coord = live && metal && ncoord >= 1;
    const bool ligpolar = live && cls == 2 && !displaced && pa >= 0;
    // the waters a receptor atom may bridge, with their box
    const bool wc = ligpolar && MR > 0;
    int wslot, wtot;
    block_compact(wc, 0, wcnt, lane, wave, wslot, wtot);
    FrameBox wb;
    if (wc) {
      wat[wslot] = make_float4(hx, hy, hz, 0.f);
      wkey[wslot] = HC_NO_KEY;
      wb.add(hx, hy, hz, 0.f);
    }
    __syncthreads();                                        // the list complete; wcnt is rewritten below
    float bd = NAN;
    int bi = -1;
    if (wtot > 0) {                                         // uniform
      wb.block_reduce(redf, lane, wave);
      const float grow = o.hbond_dist + HC_MARGIN;
      for (int b0 = 0; b0 < MR; b0 += HC_THREADS) {
        const int b = b0 + tid;
        if (b >= MR || *rec.sel(b, ppol, spol) == 0) continue;
        const float* y = rec.pos(b);
        const float yx = y[0], yy = y[1], yz = y[2];
        if (!wb.touches(yx, yy, yz, grow)) continue;
        for (int j = 0; j < wtot; ++j) {
          const float4 w = wat[j];
          const float d = sqrtf(hc_dist2(w.x, w.y, w.z, yx, yy, yz));
          if (d <= o.hbond_dist) atomicMin(&wkey[j], hc_key(d, b));
        }
      }
      __syncthreads();                                      // every key final
      if (wc) {
        const unsigned long long kb = wkey[wslot];
        if (kb != HC_NO_KEY) {
          bi = (int)(unsigned)(kb & 0xffffffffull);
          bd = __uint_as_float((unsigned)(kb >> 32));
        }
      }
    }
    const bool bridge = bi >= 0;
    const int bits = (int)clash | (int)displaced << 1 | (int)coord << 2 | (int)ligpolar << 3 | (int)bridge << 4;
    ndis += displaced; nbr += bridge; nco += coord;
    const bool emit = (bits & 23) != 0;
    int slot, tot;
    block_compact(emit, nev, wcnt, lane, wave, slot, tot);  // (its barrier: the keys are read before the next tile rewrites them)
    if (emit && slot < K) {
      const size_t e = (size_t)f * K + slot;
      if (out.event_i) {
        int32_t* ei = out.event_i + 6 * e;
        ei[0] = h; ei[1] = bits; ei[2] = amin; ei[3] = ncoord; ei[4] = ligpolar ? pa : -1; ei[5] = bi;
      }
      if (out.event_f) {
        float* ef = out.event_f + 3 * e;
        ef[0] = dmin; ef[1] = rho; ef[2] = bd;
      }
    }
    nev += tot;
    __syncthreads();                                        // wcnt is rewritten below
    block_compact(lc, ncand, wcnt, lane, wave, slot, tot);
    if (lc && slot < a.cap) {                               // a full list drops the entry: `spill` below sends the lattice passes to memory
      cand[slot] = make_float4(hx, hy, hz, Rh * Rh);
      ccls[slot] = cls;
    }
    ncand += tot;
    __syncthreads();                                        // wcnt is rewritten by the next tile
  }
  if (tid >= min(nev, K) && tid < K) {                      // the slots not used
    const size_t e = (size_t)f * K + tid;
    if (out.event_i)
      for (int q = 0; q < 6; ++q) out.event_i[6 * e + q] = -1;
    if (out.event_f)
      for (int q = 0; q < 3; ++q) out.event_f[3 * e + q] = NAN;
  }
  const bool spill = ncand > a.cap;                         // uniform: the lattice passes read every hetero atom instead
  const int ncheck = spill ? 0 : ncand;
  // lattice passes: one per distinct scale, for every class that has it
  int nvl0 = 0, nvl1 = 0, nvl2 = 0, nov0 = 0, nov1 = 0, nov2 = 0;
#pragma unroll
  for (int c0 = 0; c0 < 3; ++c0) {
    const float vs = c0 == 0 ? vs0 : (c0 == 1 ? vs1 : vs2);
    if ((c0 >= 1 && vs == vs0) || (c0 == 2 && vs == vs1)) continue;       // done with an earlier class
    const unsigned mask = 1u << c0 | (c0 < 1 && vs1 == vs ? 2u : 0u) | (c0 < 2 && vs2 == vs ? 4u : 0u);
    __syncthreads();                                        // the pass before is through with nbm
    for (int t = tid; t < 4 * N; t += HC_THREADS) {         // neighbour masks of the lattice ownership test
      const int i = t >> 2, w = t & 3;
      const float4 q = lx[i];
      const float Ri = vs * q.w;
      unsigned long long m = 0ull;
      for (int j = 0; j < 64; ++j) {
        const int c = w * 64 + j;
        if (c >= i) break;
        const float4 qc = lx[c];
        const float lim = Ri + vs * qc.w + HC_MARGIN;
        if (hc_dist2(q.x, q.y, q.z, qc.x, qc.y, qc.z) < lim * lim) m |= 1ull << j;
      }
      nbm[i][w] = m;
    }
    __syncthreads();                                        // nbm (and, the first time, cand) complete
    for (int i = 0; i < N; ++i) {
      const float4 q = lx[i];
      const float Ri = vs * q.w, R2 = Ri * Ri;
      const int x0 = (int)floorf((q.x - Ri) / hg), y0 = (int)floorf((q.y - Ri) / hg), z0 = (int)floorf((q.z - Ri) / hg);
      const int nx = (int)ceilf((q.x + Ri) / hg) - x0 + 1, ny = (int)ceilf((q.y + Ri) / hg) - y0 + 1,
                nz = (int)ceilf((q.z + Ri) / hg) - z0 + 1;
      const int B = nx * ny * nz;
      for (int t = tid; t < B; t += HC_THREADS) {
        const int ix = t % nx, iy = (t / nx) % ny, iz = t / (nx * ny);
        const float px = (float)(x0 + ix) * hg, py = (float)(y0 + iy) * hg, pz = (float)(z0 + iz) * hg;
        if (!(hc_dist2(px, py, pz, q.x, q.y, q.z) < R2)) continue;
        bool owned = true;
        for (int w = 0; w < 4 && owned; ++w) {
          unsigned long long m = nbm[i][w];
          while (m) {
            const int c = w * 64 + __ffsll((long long)m) - 1;
            m &= m - 1ull;
            const float4 qc = lx[c];
            const float Rc = vs * qc.w;
            if (hc_dist2(px, py, pz, qc.x, qc.y, qc.z) < Rc * Rc) { owned = false; break; }
          }
        }
        if (!owned) continue;
        nvl0 += mask & 1u; nvl1 += mask >> 1 & 1u; nvl2 += mask >> 2 & 1u;
        unsigned hit = 0u;
        for (int j = 0; j < ncheck && hit != mask; ++j) {
          const unsigned cb = 1u << ccls[j];
          if (!(mask & cb) || (hit & cb)) continue;
          const float4 e = cand[j];
          if (hc_dist2(px, py, pz, e.x, e.y, e.z) < e.w) hit |= cb;
        }
        if (spill)
          for (int h = 0; h < H && hit != mask; ++h) {
            const int cl = hcls[h];
            const unsigned cb = 1u << cl;
            if (!(mask & cb) || (hit & cb)) continue;
            const float Rb = (cl == 0 ? vs0 : (cl == 1 ? vs1 : vs2)) * hrad[h];
            if (hc_dist2(px, py, pz, hp[3 * (size_t)h], hp[3 * (size_t)h + 1], hp[3 * (size_t)h + 2]) < Rb * Rb) hit |= cb;
          }
        nov0 += hit & 1u; nov1 += hit >> 1 & 1u; nov2 += hit >> 2 & 1u;
      }
    }
  }
  // reductions: minima and integer sums, exact in any order
  md0 = wave_min(md0); md1 = wave_min(md1); md2 = wave_min(md2);
  key0 = hc_wave_min(key0); key1 = hc_wave_min(key1); key2 = hc_wave_min(key2);
  ncl0 = wave_sum(ncl0); ncl1 = wave_sum(ncl1); ncl2 = wave_sum(ncl2);
  ndis = wave_sum(ndis); nbr = wave_sum(nbr); nco = wave_sum(nco);
  nvl0 = wave_sum(nvl0); nvl1 = wave_sum(nvl1); nvl2 = wave_sum(nvl2);
  nov0 = wave_sum(nov0); nov1 = wave_sum(nov1); nov2 = wave_sum(nov2);
  __syncthreads();                                          // redf was read by the last tile's box
  if (lane == 0) {
    redf[wave][0] = md0; redf[wave][1] = md1; redf[wave][2] = md2;
    redk[wave][0] = key0; redk[wave][1] = key1; redk[wave][2] = key2;
    redi[wave][0] = ncl0; redi[wave][1] = ncl1; redi[wave][2] = ncl2;
    redi[wave][3] = nvl0; redi[wave][4] = nvl1; redi[wave][5] = nvl2;
    redi[wave][6] = nov0; redi[wave][7] = nov1; redi[wave][8] = nov2;
    redi[wave][9] = ndis; redi[wave][10] = nbr; redi[wave][11] = nco;
  }
  __syncthreads();
  if (tid < 4) {                                            // thread c < 3: class c (thread 3 only takes part in the shuffles)
    const int c = min(tid, 2);
    float md = INFINITY;
    unsigned long long key = HC_EMPTY_KEY;
    int ncl = 0, nvl = 0, nov = 0;
    for (int w = 0; w < HC_WAVES; ++w) {
      md = fminf(md, redf[w][c]);
      key = hc_min(key, redk[w][c]);
      ncl += redi[w][c];
      nvl += redi[w][3 + c];
      nov += redi[w][6 + c];
    }
    const float minr = __uint_as_float((unsigned)(key >> 32));
    const float vmax = c == 0 ? o.vol_overlap_max[0] : (c == 1 ? o.vol_overlap_max[1] : o.vol_overlap_max[2]);
    int pass = tid < 3 ? (int)(minr >= o.clash_ratio) << c | (int)((double)nov <= (double)vmax * (double)nvl) << (3 + c) : 0;
    pass |= __shfl_xor(pass, 1);                            // lanes 0..3 of wave 0: lane 0 ends with all six bits
    pass |= __shfl_xor(pass, 2);
    const size_t q = 3 * (size_t)f + c;
    if (tid < 3) {
      if (out.min_dist) out.min_dist[q] = md;
      if (out.min_ratio) out.min_ratio[q] = minr;
      if (out.worst) out.worst[q] = (int)(unsigned)(key & 0xffffffffull);
      if (out.n_clash) out.n_clash[q] = ncl;
      if (out.vol_lig) out.vol_lig[q] = nvl;
      if (out.vol_overlap) out.vol_overlap[q] = nov;
    }
    if (tid == 0) {
      int nd = 0, nb = 0, nc = 0;
      for (int w = 0; w < HC_WAVES; ++w) { nd += redi[w][9]; nb += redi[w][10]; nc += redi[w][11]; }
      pass |= (int)(pass == 63) << 6;
      if (out.n_displaced) out.n_displaced[f] = nd;
      if (out.n_bridge) out.n_bridge[f] = nb;
      if (out.n_coord) out.n_coord[f] = nc;
      if (out.passed) out.passed[f] = pass;
      if (out.n_event) out.n_event[f] = nev;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
static const char* HC_FN = "dbfr_hetero_check";

// the host copies of the index arrays, when the caller has them: every count, flag, class, radius and residue column
static int hc_validate(const dbfr_hetero_check_in& d, const dbfr_hetero_check_in& h) {
  if (!h.frame_ptr || !h.lig_ptr || !h.lig_rad || !h.lig_cov || !h.lig_flags || !h.het_ptr || !h.het_rad || !h.het_cov || !h.het_class ||
      !h.het_metal || !h.pocket_ptr || !h.pocket_polar || !h.pocket_col || !h.res_ptr ||
      (d.static_ptr && (!h.static_ptr || !h.static_polar || !h.static_col)))
    return arg_err(HC_FN, "host: a host copy of an index array is missing");
  const int G = d.n_group;
  if (const int rc = frame_ptr_err(HC_FN, h.frame_ptr, G, d.n_frame)) return rc;
  std::vector<float> unit;                                  // the receptor carries no radii here: the shared walk gets 1 A for each
  for (int g = 0; g < G; ++g) {
    const std::string where = "group " + std::to_string(g) + ": ";
    const int n0 = h.lig_ptr[g], N = h.lig_ptr[g + 1] - n0, h0 = h.het_ptr[g], H = h.het_ptr[g + 1] - h0, m0 = h.pocket_ptr[g],
              M = h.pocket_ptr[g + 1] - m0, s0 = d.static_ptr ? h.static_ptr[g] : 0, S = d.static_ptr ? h.static_ptr[g + 1] - s0 : 0,
              NR = h.res_ptr[g + 1] - h.res_ptr[g];
    if (const int rc = group_counts_err(HC_FN, where, {{h.frame_ptr[g + 1] - h.frame_ptr[g]}, {N, "ligand atoms", "max_lig", d.max_lig}, {H},
                                                       {M, "pocket atoms", "max_pocket", d.max_pocket}, {S},
                                                       {NR, "residue columns", "max_res", d.max_res}}))
      return rc;
    if (N < 1) return arg_err(HC_FN, where + "no ligand atoms");
    for (int i = 0; i < N; ++i) {
      if (!(h.lig_rad[n0 + i] > 0.f && h.lig_rad[n0 + i] <= 4.f) || !(h.lig_cov[n0 + i] > 0.f && h.lig_cov[n0 + i] <= 4.f))
        return arg_err(HC_FN, where + "the radius of ligand atom " + std::to_string(i) + " lies outside (0, 4]");
      if (h.lig_flags[n0 + i] > 3) return arg_err(HC_FN, where + "the flags of ligand atom " + std::to_string(i) + " hold an unknown bit");
    }
    for (int i = 0; i < H; ++i) {
      if (h.het_class[h0 + i] > 2) return arg_err(HC_FN, where + "the class of hetero atom " + std::to_string(i) + " is not 0, 1 or 2");
      if (!(h.het_rad[h0 + i] > 0.f && h.het_rad[h0 + i] <= 4.f) || !(h.het_cov[h0 + i] > 0.f && h.het_cov[h0 + i] <= 4.f))
        return arg_err(HC_FN, where + "the radius of hetero atom " + std::to_string(i) + " lies outside (0, 4]");
    }
    if (unit.size() < (size_t)std::max(M, S)) unit.assign((size_t)std::max(M, S), 1.f);
    if (const int rc = receptor_atoms_err(HC_FN, where, M, S, unit.data(), unit.data(), h.pocket_col + m0,
                                          d.static_ptr ? h.static_col + s0 : nullptr, NR, [](int) { return DBFR_OK; }))
      return rc;
  }
  return DBFR_OK;
}

extern "C" int dbfr_hetero_check(const dbfr_hetero_check_in* in, const dbfr_hetero_check_opts* opts, const dbfr_hetero_check_out* out,
                                 void* hip_stream) {
  const char* fn = HC_FN;
  if (!in || !out) return arg_err(fn, "null argument");
  if (in->n_group < 0 || in->n_frame < 0) return arg_err(fn, "negative n_group / n_frame");
  if (in->max_lig < 0 || in->max_lig > HC_MAX_LIG) return limit_err(fn, "max_lig (ligand atoms)", in->max_lig, 0, HC_MAX_LIG);
  if (in->max_pocket < 0 || in->max_pocket > HC_MAX_POCKET) return limit_err(fn, "max_pocket (pocket atoms)", in->max_pocket, 0, HC_MAX_POCKET);
  if (in->max_res < 0 || in->max_res > HC_MAX_RES) return limit_err(fn, "max_res (residue columns)", in->max_res, 0, HC_MAX_RES);
  if (in->cand_cap < 0 || in->cand_cap > HC_CAND) return limit_err(fn, "cand_cap (LDS lattice candidates)", in->cand_cap, 0, HC_CAND);
  dbfr_hetero_check_opts o = {0.75f, 2.0f, 2.8f, 3.5f, 0.25f, {0.8f, 0.5f, 0.5f}, {0.075f, 0.075f, 0.075f}, 32};
  if (opts) o = *opts;
  if (o.max_event < 1 || o.max_event > HC_MAX_EVENT) return limit_err(fn, "max_event (events kept per frame)", o.max_event, 1, HC_MAX_EVENT);
  if (!(o.grid >= 0.05f && o.grid <= 1.f)) return arg_err(fn, "grid must lie in [0.05, 1] A");
  for (int c = 0; c < 3; ++c) {
    if (!(o.vol_scale[c] > 0.f && o.vol_scale[c] <= 2.f)) return arg_err(fn, "vol_scale must lie in (0, 2]");
    if (std::isnan(o.vol_overlap_max[c])) return arg_err(fn, "a threshold is NaN");
  }
  if (!(o.hbond_dist > 0.f && o.hbond_dist <= 8.f)) return arg_err(fn, "hbond_dist must lie in (0, 8] A");
  if (std::isnan(o.clash_ratio) || std::isnan(o.displace_dist) || std::isnan(o.metal_dist)) return arg_err(fn, "a threshold is NaN");
  if (in->n_frame == 0) return DBFR_OK;
  if (in->n_group == 0) return arg_err(fn, "frames without groups");
  if (!in->frame_ptr || !in->lig_ptr || !in->lig_pos_off || !in->lig_pos || !in->lig_rad || !in->lig_cov || !in->lig_flags || !in->het_ptr ||
      !in->het_pos || !in->het_rad || !in->het_cov || !in->het_class || !in->het_metal || !in->pocket_ptr || !in->pocket_pos_off ||
      !in->pocket_pos || !in->pocket_polar || !in->pocket_col || !in->res_ptr)
    return arg_err(fn, "frame_ptr / lig_ptr / lig_pos_off / lig_pos / lig_rad / lig_cov / lig_flags / het_ptr / het_pos / het_rad / het_cov / "
                       "het_class / het_metal / pocket_ptr / pocket_pos_off / pocket_pos / pocket_polar / pocket_col / res_ptr missing");
  if (in->static_ptr && (!in->static_pos || !in->static_polar || !in->static_col))
    return arg_err(fn, "static_ptr given without static_pos / static_polar / static_col");
  if (in->host) {
    const int rc = hc_validate(*in, *static_cast<const dbfr_hetero_check_in*>(in->host));
    if (rc != DBFR_OK) return rc;
  }
  HcArgs a;
  a.in = *in;
  a.in.host = nullptr;
  a.o = o;
  a.out = *out;
  a.cap = in->cand_cap ? in->cand_cap : HC_CAND;
  HIPCHECK(launch_frames(k_hetero_check, in->n_frame, HC_THREADS, 0, hip_stream, a));
  return DBFR_OK;
}
