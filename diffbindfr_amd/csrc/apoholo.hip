// Holo-pocket recovery of apo / AF2 docking: the sequence alignment (host), the binding-site selection and, for every frame of a
// ragged batch, the side-chain RMSD, chi angles and lDDT-style pocket / ligand distance scores against the holo structure.
// include/dbfr.h states the definitions; docs/apoholo.md the layout, the limits and the deviations from the reference.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dbfr.h"
#include "common.h"
#include "frames.h"

#define RT_TABLE __device__ const
namespace ah_tables {
#include "residue_tables.inc"
}
#undef RT_TABLE

#define AH_THREADS FR_THREADS
#define AH_WAVES FR_WAVES
#define AH_PERM_TILE 256           // automorphisms whose numerators sit in LDS at a time
#define AH_MAX_RES (DBFR_HOLO_MAX_POCKET / 14)
#define AH_VAL 19
#define AH_SIDE 0x3FF0u            // atom14 slots 4..13: the heavy atoms but N, CA, C, O

struct AhArgs {
  dbfr_holo_metrics_in in;
  dbfr_holo_metrics_out out;
  float radius;
};

__device__ __forceinline__ float ah_dist(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return sqrtf(dx * dx + dy * dy + dz * dz);
}

// ------------------------------------------------------------------------------------------------ the pairs of a group
// One wave per site residue: the holo distance of every (atom14 slot, holo ligand atom) pair and whether it is scored.
__global__ __launch_bounds__(64) void k_holo_pairs(AhArgs a) {
  const dbfr_holo_metrics_in& in = a.in;
  const int sf = blockIdx.x, lane = threadIdx.x;
  const int g = frame_group(in.site_ptr, in.n_group, sf);
  const int s = sf - in.site_ptr[g], S = in.site_ptr[g + 1] - in.site_ptr[g];
  const int h0 = in.hlig_ptr[g], H = in.hlig_ptr[g + 1] - h0;
  int cnt = 0;
  if (S <= in.max_site && H >= 0 && H <= in.max_lig) {
    const bool matched = in.site_matched[sf] != 0;
    float* dst = a.out.pair_dist + in.pair_off[g] + (long long)s * 14 * H;
    const float* x = in.holo14 + 42 * (size_t)sf;
    for (int idx = lane; idx < 14 * H; idx += 64) {
      const int at = idx / H, h = idx - at * H;
      const bool ok = matched && in.holo_mask[14 * (size_t)sf + at] && in.frame_mask[14 * (size_t)sf + at];
      const float* y = in.hlig + 3 * (size_t)(h0 + h);
      const float d = ah_dist(x[3 * at], x[3 * at + 1], x[3 * at + 2], y[0], y[1], y[2]);
      const bool scored = ok && d < a.radius;               // false for a NaN distance
      dst[idx] = scored ? d : -1.f;
      cnt += scored;
    }
  }
  cnt = wave_sum(cnt);
  if (lane == 0) {
    if (a.out.plddt_den) a.out.plddt_den[sf] = cnt;
    if (a.out.lddt_den && cnt) atomicAdd(&a.out.lddt_den[g], cnt);        // an integer sum: the order does not matter
  }
}

// ------------------------------------------------------------------------------------------------ the frames
// the dihedral p0-p1-p2-p3, IUPAC sign: atan2(|b2| b1 . (b2 x b3), (b1 x b2) . (b2 x b3))
__device__ __forceinline__ float ah_dihedral(const float* p0, const float* p1, const float* p2, const float* p3) {
  const float b1x = p1[0] - p0[0], b1y = p1[1] - p0[1], b1z = p1[2] - p0[2];
  const float b2x = p2[0] - p1[0], b2y = p2[1] - p1[1], b2z = p2[2] - p1[2];
  const float b3x = p3[0] - p2[0], b3y = p3[1] - p2[1], b3z = p3[2] - p2[2];
  const float n1x = b1y * b2z - b1z * b2y, n1y = b1z * b2x - b1x * b2z, n1z = b1x * b2y - b1y * b2x;
  const float n2x = b2y * b3z - b2z * b3y, n2y = b2z * b3x - b2x * b3z, n2z = b2x * b3y - b2y * b3x;
  const float l2 = sqrtf(b2x * b2x + b2y * b2y + b2z * b2z);
  const float y = l2 * (b1x * n2x + b1y * n2y + b1z * n2z), x = n1x * n2x + n1y * n2y + n1z * n2z;
  return atan2f(y, x);
}

__device__ __forceinline__ float ah_wrap(float d) {          // |d| for d in (-2 pi, 2 pi) wrapped into [0, pi]; NaN stays
  const float pi = 3.14159265358979323846f, two_pi = 6.28318530717958647692f;
  d = fabsf(d);
  return d > pi ? two_pi - d : d;
}

// One workgroup per frame.  The frame's pocket rows, the holo ligand and the pose's ligand are read once and sit in LDS; then one
// wave per site residue: lanes 4..13 the side-chain atoms, lanes 0..5 the dihedrals, all lanes the (atom, ligand atom) pairs of the
// group's pair table.  Counts are integer sums; the side-chain sum of a residue runs over the slots in order and the pooled sum
// over the residues in a fixed tree: nothing depends on the launch.
__global__ __launch_bounds__(AH_THREADS) void k_holo_frames(AhArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ah_dyn[];      // pocket [R, 42], holo ligand [H, 3], ligand [N, 3], sq [S], n [S]
  __shared__ int permacc[AH_PERM_TILE];
  __shared__ int best_s;
  const dbfr_holo_metrics_in& in = a.in;
  const dbfr_holo_metrics_out& out = a.out;
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = frame_group(in.frame_ptr, in.n_group, f);
  const int k = f - in.frame_ptr[g];
  const int s0 = in.site_ptr[g], S = in.site_ptr[g + 1] - s0;
  const int R = in.res_ptr[g + 1] - in.res_ptr[g];
  const int h0 = in.hlig_ptr[g], H = in.hlig_ptr[g + 1] - h0;
  const int N = in.lig_ptr[g + 1] - in.lig_ptr[g];
  const int n_perm = in.perm_ptr[g + 1] - in.perm_ptr[g];
  const bool shape_ok = S >= 0 && S <= in.max_site && R >= 0 && R <= in.max_res && H >= 0 && H <= in.max_lig && N >= 0 && N <= in.max_lig;
  float* pk = ah_dyn;
  float* hl = pk + 42 * (shape_ok ? R : 0);
  float* pl = hl + 3 * (shape_ok ? H : 0);
  float* sq = pl + 3 * (shape_ok ? N : 0);
  int* sn = reinterpret_cast<int*>(sq + (shape_ok ? S : 0));
  const long long orow = in.site_off[g] + (long long)k * S;          // the frame's first per-residue output row
  int bad_x = 0;
  if (shape_ok) {
    const float* src = in.pocket + 42 * (in.pocket_off[g] + (long long)k * R);
    for (int i = tid; i < 42 * R; i += AH_THREADS) {
      const float v = src[i];
      bad_x |= !coord_ok(v);
      pk[i] = v;
    }
    for (int i = tid; i < 3 * H; i += AH_THREADS) hl[i] = in.hlig[3 * (size_t)h0 + i];
    const float* lsrc = in.lig + 3 * (in.lig_off[g] + (long long)k * N);
    for (int i = tid; i < 3 * N; i += AH_THREADS) {
      const float v = lsrc[i];
      bad_x |= !coord_ok(v);
      pl[i] = v;
    }
    for (int i = tid; i < 42 * S; i += AH_THREADS) {                  // the static atoms that stand in for a pocket row
      const int s = i / 42;
      if (in.site_matched[s0 + s] && in.site_row[s0 + s] < 0 && in.frame_mask[14 * (size_t)(s0 + s) + (i - 42 * s) / 3])
        bad_x |= !coord_ok(in.apo14[42 * (size_t)s0 + i]);
    }
    for (int s = tid; s < S; s += AH_THREADS) {
      sq[s] = 0.f;
      sn[s] = 0;
    }
  }
  if (tid == 0) best_s = -1;
  const bool bad = __syncthreads_or(bad_x) || !shape_ok;              // uniform over the workgroup; LDS complete
  const float nan = __builtin_nanf("");
  if (bad) {
    if (shape_ok)
      for (int s = tid; s < S; s += AH_THREADS) {
        if (out.sc_rmsd) out.sc_rmsd[orow + s] = nan;
        if (out.plddt_num) out.plddt_num[orow + s] = -1;
        for (int c = 0; c < 4; ++c) {
          if (out.chi) out.chi[4 * (orow + s) + c] = nan;
          if (out.dchi) out.dchi[4 * (orow + s) + c] = nan;
        }
        if (out.altchi) out.altchi[2 * (orow + s)] = out.altchi[2 * (orow + s) + 1] = nan;
      }
    if (tid == 0) {
      if (out.sc_sq_sum) out.sc_sq_sum[f] = nan;
      if (out.sc_n) out.sc_n[f] = -1;
      if (out.lddt_num) out.lddt_num[f] = -1;
    }
    return;
  }
  const bool do_lddt = N == H && H > 0 && n_perm > 0;
  const int32_t* perms = in.perms + in.perm_off[g];
  const float* pd = out.pair_dist + in.pair_off[g];
  for (int p0 = 0; p0 < (do_lddt ? n_perm : 1); p0 += AH_PERM_TILE) {
    const int np = do_lddt ? min(AH_PERM_TILE, n_perm - p0) : 0;
    permacc[tid] = 0;
    __syncthreads();
    for (int s = wave; s < S; s += AH_WAVES) {
      const size_t sf = (size_t)(s0 + s);
      const bool matched = in.site_matched[sf] != 0;
      int row = in.site_row[sf];
      if (row >= R) row = R - 1;                                      // (refused on the host; never read beyond the frame)
      const float* stat = in.apo14 + 42 * sf;
      auto X = [&](int at, int c) -> float { return row >= 0 ? pk[42 * row + 3 * at + c] : stat[3 * at + c]; };
      const unsigned hmask = (unsigned)__ballot(lane < 14 && in.holo_mask[14 * sf + min(lane, 13)]);
      const unsigned fmask = (unsigned)__ballot(lane < 14 && in.frame_mask[14 * sf + min(lane, 13)]);
      const float* base = pd + (long long)s * 14 * H;
      if (p0 == 0) {
        // side chain: lanes 4..13 one atom each, lane 0 adds them in slot order
        const bool paired = matched && (hmask & AH_SIDE) == (fmask & AH_SIDE) && (hmask & AH_SIDE) != 0;
        float d2 = 0.f;
        if (lane >= 4 && lane < 14 && ((hmask >> lane) & 1u)) {
          const float* hx = in.holo14 + 42 * sf + 3 * lane;
          const float dx = hx[0] - X(lane, 0), dy = hx[1] - X(lane, 1), dz = hx[2] - X(lane, 2);
          d2 = dx * dx + dy * dy + dz * dz;
        }
        float sum = 0.f;
        for (int at = 4; at < 14; ++at) {
          const float v = __shfl(d2, at);
          if ((hmask >> at) & 1u) sum += v;
        }
        const int n_sc = __popc(hmask & AH_SIDE);
        if (lane == 0) {
          if (out.sc_rmsd) out.sc_rmsd[orow + s] = paired ? sqrtf(sum / (float)n_sc) : nan;
          sq[s] = paired ? sum : 0.f;
          sn[s] = paired ? n_sc : 0;
        }
        // dihedrals: lanes 0..3 chi1..chi4, lane 4 altchi1, lane 5 altchi2
        const int aa = in.site_aatype[sf];
        float ang = nan;
        if (lane < 6 && matched && aa >= 0 && aa < 20) {
          const int kx = lane < 4 ? lane : lane - 4;
          const bool alt_ok = lane == 4 ? aa == AH_VAL : (aa == 3 || aa == 10 || aa == 13 || aa == 18);     // ASP, LEU, PHE, TYR
          if (ah_tables::kChiMask[aa][kx] && (lane < 4 || alt_ok)) {
            const int i0 = ah_tables::kChiAtoms14[aa][kx][0], i1 = ah_tables::kChiAtoms14[aa][kx][1], i2 = ah_tables::kChiAtoms14[aa][kx][2],
                      i3 = ah_tables::kChiAtoms14[aa][kx][3] + (lane >= 4 ? 1 : 0);
            if (((fmask >> i0) & (fmask >> i1) & (fmask >> i2) & (fmask >> i3)) & 1u) {
              const float q0[3] = {X(i0, 0), X(i0, 1), X(i0, 2)}, q1[3] = {X(i1, 0), X(i1, 1), X(i1, 2)},
                          q2[3] = {X(i2, 0), X(i2, 1), X(i2, 2)}, q3[3] = {X(i3, 0), X(i3, 1), X(i3, 2)};
              ang = ah_dihedral(q0, q1, q2, q3);
            }
          }
        }
        const float alt = __shfl(ang, lane == 0 ? 4 : 5);
        if (lane < 4) {
          if (out.chi) out.chi[4 * (orow + s) + lane] = ang;
          if (out.dchi) {
            const float hc = in.holo_chi[4 * sf + lane];
            float d = ah_wrap(ang - hc);
            if (lane < 2 && alt == alt && d == d) d = fminf(d, ah_wrap(alt - hc));
            out.dchi[4 * (orow + s) + lane] = d;
          }
        } else if (lane < 6 && out.altchi) {
          out.altchi[2 * (orow + s) + lane - 4] = ang;
        }
        // pocket-atom / holo-ligand-atom distances against the holo's
        int cnt = 0;
        if (matched)
          for (int idx = lane; idx < 14 * H; idx += 64) {
            const float dh = base[idx];
            if (dh >= 0.f) {
              const int at = idx / H, h = idx - at * H;
              const float df = fabsf(dh - ah_dist(X(at, 0), X(at, 1), X(at, 2), hl[3 * h], hl[3 * h + 1], hl[3 * h + 2]));
              cnt += (df < 0.5f) + (df < 1.f) + (df < 2.f) + (df < 4.f);
            }
          }
        cnt = wave_sum(cnt);
        if (lane == 0 && out.plddt_num) out.plddt_num[orow + s] = cnt;
      }
      // the same against the pose's own ligand, one numerator per automorphism
      if (matched)
        for (int p = 0; p < np; ++p) {
          const int32_t* pm = perms + (long long)(p0 + p) * N;
          int cnt = 0;
          for (int idx = lane; idx < 14 * H; idx += 64) {
            const float dh = base[idx];
            if (dh >= 0.f) {
              const int at = idx / H, h = idx - at * H;
              const int n = min(max(pm[h], 0), N - 1);
              const float df = fabsf(dh - ah_dist(X(at, 0), X(at, 1), X(at, 2), pl[3 * n], pl[3 * n + 1], pl[3 * n + 2]));
              cnt += (df < 0.5f) + (df < 1.f) + (df < 2.f) + (df < 4.f);
            }
          }
          cnt = wave_sum(cnt);
          if (lane == 0 && cnt) atomicAdd(&permacc[p], cnt);            // an integer sum in LDS
        }
    }
    __syncthreads();                                                  // every numerator of the tile, sq and sn complete
    if (tid < np) atomicMax(&best_s, permacc[tid]);
    __syncthreads();                                                  // permacc is zeroed by the next tile
  }
  // the pooled side-chain sum: lane l adds residues l, l + 64, ... in order, then a fixed tree over the lanes
  if (wave == 0) {
    float v = 0.f;
    int n = 0;
    for (int s = lane; s < S; s += 64) {
      v += sq[s];
      n += sn[s];
    }
    for (int o = 32; o > 0; o >>= 1) {
      v += __shfl_down(v, o, 64);
      n += __shfl_down(n, o, 64);
    }
    if (lane == 0) {
      if (out.sc_sq_sum) out.sc_sq_sum[f] = v;
      if (out.sc_n) out.sc_n[f] = n;
      if (out.lddt_num) out.lddt_num[f] = do_lddt ? best_s : -1;
    }
  }
}

// ------------------------------------------------------------------------------------------------ the binding site
// One thread per listed atom, the ligand in LDS tiles of 256 atoms.  Every flagged residue receives the same byte from every
// thread that flags it.
__global__ __launch_bounds__(AH_THREADS) void k_holo_site(dbfr_holo_site_in in, uint8_t* site) {
  __shared__ float lig[3 * AH_THREADS];
  const int p = blockIdx.y, tid = threadIdx.x;
  const int a0 = in.atom_ptr[p], A = in.atom_ptr[p + 1] - a0;
  if ((int)(blockIdx.x * AH_THREADS) >= A) return;                    // uniform over the workgroup
  const int l0 = in.lig_ptr[p], NL = in.lig_ptr[p + 1] - l0;
  const int r0 = in.res_ptr[p], NR = in.res_ptr[p + 1] - r0;
  const int i = blockIdx.x * AH_THREADS + tid;
  const bool live = i < A;
  float x = 0.f, y = 0.f, z = 0.f;
  int res = -1;
  if (live) {
    const float* q = in.atom_pos + 3 * (size_t)(a0 + i);
    x = q[0]; y = q[1]; z = q[2];
    res = in.atom_res[a0 + i];
  }
  bool hit = false;
  for (int t0 = 0; t0 < NL; t0 += AH_THREADS) {
    const int nt = min(AH_THREADS, NL - t0);
    __syncthreads();                                                  // the previous tile is read
    for (int j = tid; j < 3 * nt; j += AH_THREADS) lig[j] = in.lig_pos[3 * (size_t)(l0 + t0) + j];
    __syncthreads();
    for (int j = 0; j < nt; ++j) hit = hit || ah_dist(x, y, z, lig[3 * j], lig[3 * j + 1], lig[3 * j + 2]) <= in.cutoff;
  }
  if (live && hit && res >= 0 && res < NR) site[r0 + res] = 1;
}

// ------------------------------------------------------------------------------------------------ host
// the longest common subsequence of a and b with the traceback of include/dbfr.h; the table in uint16 (a score is <= 8192)
static int ah_align_one(const int32_t* a, int na, const int32_t* b, int nb, int32_t* a_to_b) {
  for (int i = 0; i < na; ++i) a_to_b[i] = -1;
  if (na == 0 || nb == 0) return 0;
  const size_t w = (size_t)nb + 1;
  std::vector<uint16_t> S((size_t)(na + 1) * w, 0);
  auto same = [&](int i, int j) { return a[i] == b[j] && a[i] >= 0 && a[i] < 20; };
  for (int i = 1; i <= na; ++i) {
    const uint16_t* up = &S[(size_t)(i - 1) * w];
    uint16_t* cur = &S[(size_t)i * w];
    for (int j = 1; j <= nb; ++j) {
      uint16_t v = std::max(up[j], cur[j - 1]);
      if (same(i - 1, j - 1)) v = std::max<uint16_t>(v, up[j - 1] + 1);
      cur[j] = v;
    }
  }
  int i = na, j = nb;
  while (i > 0 && j > 0) {
    const uint16_t v = S[(size_t)i * w + j];
    if (same(i - 1, j - 1) && v == S[(size_t)(i - 1) * w + j - 1] + 1) {
      a_to_b[i - 1] = j - 1;
      --i;
      --j;
    } else if (S[(size_t)(i - 1) * w + j] == v) {
      --i;
    } else {
      --j;
    }
  }
  return S[(size_t)na * w + nb];
}

extern "C" int dbfr_seq_align(int32_t n_pair, const int32_t* a_ptr, const int32_t* a, const int32_t* b_ptr, const int32_t* b,
                              int32_t* a_to_b, int32_t* score, int32_t n_threads) {
  const char* fn = "dbfr_seq_align";
  if (n_pair < 0) return arg_err(fn, "negative n_pair");
  if (n_pair == 0) return DBFR_OK;
  if (!a_ptr || !b_ptr || !a_to_b) return arg_err(fn, "a_ptr / b_ptr / a_to_b missing");
  for (int p = 0; p < n_pair; ++p) {
    const long long na = (long long)a_ptr[p + 1] - a_ptr[p], nb = (long long)b_ptr[p + 1] - b_ptr[p];
    if (na < 0 || nb < 0) return arg_err(fn, "pair " + std::to_string(p) + ": a negative length");
    if (na * nb > DBFR_ALIGN_MAX_CELLS)
      return arg_err(fn, "pair " + std::to_string(p) + ": " + std::to_string(na) + " x " + std::to_string(nb) + " cells, at most 2^26");
    if ((na && !a) || (nb && !b)) return arg_err(fn, "a / b missing");
  }
  int nt = n_threads > 0 ? n_threads : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  nt = std::min(nt, (int)n_pair);
  std::atomic<int> next(0);
  auto work = [&]() {
    for (int p = next++; p < n_pair; p = next++) {
      const int sc = ah_align_one(a + a_ptr[p], a_ptr[p + 1] - a_ptr[p], b + b_ptr[p], b_ptr[p + 1] - b_ptr[p], a_to_b + a_ptr[p]);
      if (score) score[p] = sc;
    }
  };
  if (nt <= 1) {
    work();
  } else {
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back(work);
    for (auto& t : th) t.join();
  }
  return DBFR_OK;
}

extern "C" int dbfr_holo_site(const dbfr_holo_site_in* in, uint8_t* site, void* hip_stream) {
  const char* fn = "dbfr_holo_site";
  if (!in || !site) return arg_err(fn, "null argument");
  if (in->n_pair < 0 || in->max_atoms < 0) return arg_err(fn, "negative n_pair / max_atoms");
  if (!(in->cutoff > 0.f && in->cutoff <= 100.f)) return arg_err(fn, "cutoff must lie in (0, 100] A and must not be NaN");
  if (in->n_pair == 0) return DBFR_OK;
  if (in->n_pair > 65535) return arg_err(fn, "more than 65535 pairs in one launch");
  if (!in->atom_ptr || !in->atom_pos || !in->atom_res || !in->lig_ptr || !in->lig_pos || !in->res_ptr)
    return arg_err(fn, "atom_ptr / atom_pos / atom_res / lig_ptr / lig_pos / res_ptr missing");
  const int32_t n_res = in->n_res;
  if (n_res < 0) return arg_err(fn, "negative n_res");
  if (n_res == 0 || in->max_atoms == 0) return DBFR_OK;
  HIPCHECK(hipMemsetAsync(site, 0, (size_t)n_res, (hipStream_t)hip_stream));
  const unsigned bx = (unsigned)((in->max_atoms + AH_THREADS - 1) / AH_THREADS);
  hipLaunchKernelGGL(k_holo_site, dim3(bx, (unsigned)in->n_pair), dim3(AH_THREADS), 0, (hipStream_t)hip_stream, *in, site);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

// the host copies of the index arrays, when the caller has them
static int ah_validate(const dbfr_holo_metrics_in& d, const dbfr_holo_metrics_in& h) {
  const char* fn = "dbfr_holo_metrics";
  if (!h.frame_ptr || !h.site_ptr || !h.site_row || !h.site_off || !h.res_ptr || !h.pocket_off || !h.hlig_ptr || !h.pair_off || !h.lig_ptr ||
      !h.lig_off || !h.perm_ptr || !h.perm_off || (h.perm_ptr[d.n_group] > 0 && !h.perms))
    return arg_err(fn, "host: a host copy of an index array is missing");
  const int G = d.n_group;
  if (const int rc = frame_ptr_err(fn, h.frame_ptr, G, d.n_frame)) return rc;
  long long site_rows = 0, pocket_rows = 0, pair_floats = 0, lig_rows = 0, perm_ints = 0;
  for (int g = 0; g < G; ++g) {
    const std::string where = "group " + std::to_string(g) + ": ";
    const long long F = (long long)h.frame_ptr[g + 1] - h.frame_ptr[g], S = (long long)h.site_ptr[g + 1] - h.site_ptr[g],
                    R = (long long)h.res_ptr[g + 1] - h.res_ptr[g], H = (long long)h.hlig_ptr[g + 1] - h.hlig_ptr[g],
                    N = (long long)h.lig_ptr[g + 1] - h.lig_ptr[g], P = (long long)h.perm_ptr[g + 1] - h.perm_ptr[g];
    if (const int rc = group_counts_err(fn, where, {{F}, {S, "site residues", "max_site", d.max_site}, {R, "pocket rows", "max_res", d.max_res},
                                                    {H}, {N}, {P}, {std::max(H, N), "ligand atoms", "max_lig", d.max_lig}}))
      return rc;
    // the arrays are laid out group by group without overlap
    if (h.site_off[g] != site_rows || h.pocket_off[g] != pocket_rows || h.pair_off[g] != pair_floats || h.lig_off[g] != lig_rows ||
        h.perm_off[g] != perm_ints)
      return arg_err(fn, where + "site_off / pocket_off / pair_off / lig_off / perm_off is not the running sum of the groups before it");
    site_rows += F * S; pocket_rows += F * R; pair_floats += S * 14 * H; lig_rows += F * N; perm_ints += P * N;
    for (int s = 0; s < S; ++s) {
      const int row = h.site_row[h.site_ptr[g] + s];
      if (row < -1 || row >= R) return arg_err(fn, where + "site_row " + std::to_string(row) + " of site residue " + std::to_string(s) + " is no pocket row");
    }
    if (N == H && H > 0 && P < 1) return arg_err(fn, where + "no automorphism (the identity is one)");
    for (long long i = 0; i < P * N; ++i)
      if (h.perms[h.perm_off[g] + i] < 0 || h.perms[h.perm_off[g] + i] >= N)
        return arg_err(fn, where + "an automorphism entry is no ligand atom");
  }
  return DBFR_OK;
}

extern "C" int dbfr_holo_metrics(const dbfr_holo_metrics_in* in, const dbfr_holo_metrics_opts* opts, const dbfr_holo_metrics_out* out,
                                 void* hip_stream) {
  const char* fn = "dbfr_holo_metrics";
  if (!in || !out) return arg_err(fn, "null argument");
  if (in->n_group < 0 || in->n_frame < 0) return arg_err(fn, "negative n_group / n_frame");
  if (in->max_site < 0 || in->max_site > DBFR_HOLO_MAX_SITE) return limit_err(fn, "max_site (site residues)", in->max_site, 0, DBFR_HOLO_MAX_SITE);
  if (in->max_res < 0 || in->max_res > AH_MAX_RES) return limit_err(fn, "14 max_res (pocket atoms)", 14LL * in->max_res, 0, DBFR_HOLO_MAX_POCKET);
  if (in->max_lig < 0 || in->max_lig > DBFR_HOLO_MAX_LIG) return limit_err(fn, "max_lig (ligand atoms)", in->max_lig, 0, DBFR_HOLO_MAX_LIG);
  dbfr_holo_metrics_opts o = {6.0f};
  if (opts) o = *opts;
  if (!(o.radius > 0.f && o.radius <= 100.f)) return arg_err(fn, "radius must lie in (0, 100] A and must not be NaN");
  if (in->n_group == 0) return in->n_frame == 0 ? DBFR_OK : arg_err(fn, "frames without groups");
  if (!in->frame_ptr || !in->site_ptr || !in->site_aatype || !in->site_row || !in->site_matched || !in->holo14 || !in->holo_mask || !in->apo14 ||
      !in->frame_mask || !in->holo_chi || !in->site_off || !in->res_ptr || !in->pocket_off || !in->pocket || !in->hlig_ptr || !in->hlig ||
      !in->pair_off || !in->lig_ptr || !in->lig_off || !in->lig || !in->perm_ptr || !in->perm_off || !in->perms)
    return arg_err(fn, "an input array is missing");
  if (!out->pair_dist) return arg_err(fn, "out.pair_dist (the pair table of every group) is missing");
  if (!in->host) return arg_err(fn, "in.host (the host copies of the index arrays) is missing: the counts are validated before every launch");
  const dbfr_holo_metrics_in& h = *static_cast<const dbfr_holo_metrics_in*>(in->host);
  const int rc = ah_validate(*in, h);
  if (rc != DBFR_OK) return rc;
  AhArgs a;
  a.in = *in;
  a.in.host = nullptr;
  a.out = *out;
  a.radius = o.radius;
  hipStream_t st = (hipStream_t)hip_stream;
  const int n_site = h.site_ptr[in->n_group];
  if (out->lddt_den) HIPCHECK(hipMemsetAsync(out->lddt_den, 0, sizeof(int32_t) * (size_t)in->n_group, st));
  if (n_site > 0) {
    HIPCHECK(launch_frames(k_holo_pairs, n_site, 64, 0, st, a));
  }
  if (in->n_frame == 0) return DBFR_OK;
  const size_t lds = 4 * (42 * (size_t)in->max_res + 6 * (size_t)in->max_lig + 2 * (size_t)in->max_site) + 16;
  HIPCHECK(launch_frames(k_holo_frames, in->n_frame, AH_THREADS, lds, st, a));
  return DBFR_OK;
}
