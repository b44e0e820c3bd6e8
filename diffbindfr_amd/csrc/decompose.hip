// Per-residue and per-ligand-atom decomposition of the Vina inter-molecular energy of poses: the five weighted terms of every
// (ligand atom, receptor atom) pair within the cutoff, summed per receptor column (a protein residue or a hetero residue), per
// ligand atom and per frame, for every frame of a ragged batch, in one launch.
// include/dbfr.h states the definitions; docs/decompose.md the layout and the limits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/dbfr.h"
#include "common.h"
#include "frames.h"
#define VINA_XS_RAD d_rad
#define VINA_XS_FLAGS d_flags
#include "vina_terms.h"

// One workgroup per frame.  The ligand (x, y, z, XS type) is staged in LDS with its bounding box.  The receptor (the frame's
// pocket atoms, then the group's static atoms: the rest of the protein and the hetero atoms) goes past in tiles of one atom per
// thread; the typed atoms inside the box grown by the cutoff are compacted in index order into an LDS list, and every full tile
// of 256 candidates (and the remainder at the end) is worked off twice: a thread per candidate walks the ligand and adds its
// five sums to its column, a thread per ligand atom walks the tile and keeps its five sums in registers.
// A pair's five fp32 terms are k_vina's: both kernels call pair_terms of csrc/vina_terms.h, which also holds the XS table and the
// typed predicate (tests/test_decompose_gpu.py compares the two kernels' totals).
// Each term is rounded once to a 64-bit integer in units of 2^-36 kcal/mol and every sum is an integer sum:
// exact in any order, so the column sums go through integer atomics on the frame's own rows, the bits of a frame do not depend on
// the launch it is part of, and sum(columns) == sum(atoms) == totals holds exactly in the integer outputs.
#define VD_THREADS FR_THREADS
#define VD_WAVES FR_WAVES
#define VD_MAX_LIG 256
#define VD_MAX_COL 16384
#define VD_FIXED 68719476736.0     // 2^36 units per kcal/mol: 1.5e-11 resolution, sums up to 1.3e8 kcal/mol
#define VD_BAD_FIXED ((long long)0x8000000000000000ull)

struct VdArgs {
  dbfr_vina_decompose_in in;
  dbfr_vina_decompose_out out;
  float cutoff;
};

// the pair (ligand atom l, receptor atom c; w = the type as int bits) added to acc[0..4] when it lies within the cutoff
__device__ __forceinline__ void vd_add_pair(const float4& l, const float4& c, float cut2, long long* acc) {
  const float dx = l.x - c.x, dy = l.y - c.y, dz = l.z - c.z;
  const float r2 = dx * dx + dy * dy + dz * dz;
  if (r2 >= cut2) return;
  float t5[5];
  pair_terms<false>(__float_as_int(l.w), __float_as_int(c.w), sqrtf(r2), t5);
#pragma unroll
  for (int k = 0; k < 5; ++k) acc[k] += __double2ll_rn((double)t5[k] * VD_FIXED);
}

__device__ __forceinline__ float vd_float(long long v) { return (float)((double)v * (1.0 / VD_FIXED)); }

__device__ __forceinline__ long long vd_wave_sum(long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)((unsigned long long)v >> 32), o);
    v += (long long)(((unsigned long long)hi << 32) | lo);
  }
  return v;
}

__global__ __launch_bounds__(VD_THREADS) void k_vina_decompose(VdArgs a) {
  __shared__ float4 lx[VD_MAX_LIG];                         // x, y, z, XS type (as int bits; -1 = takes part in no term)
  __shared__ float4 cx[2 * VD_THREADS];                     // the candidate list: x, y, z, XS type (as int bits)
  __shared__ int ccol[2 * VD_THREADS];                      // their columns
  __shared__ int wcnt[VD_WAVES];
  __shared__ float redf[VD_WAVES][8];
  __shared__ long long redt[VD_WAVES][5];
  const dbfr_vina_decompose_in& in = a.in;
  const dbfr_vina_decompose_out& out = a.out;
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = frame_group(in.frame_ptr, in.n_group, f);
  const int k = f - in.frame_ptr[g];
  const int l0 = in.lig_ptr[g], N = in.lig_ptr[g + 1] - l0;
  const int m0 = in.pocket_ptr[g], M = in.pocket_ptr[g + 1] - m0;
  const int s0 = in.static_ptr ? in.static_ptr[g] : 0, S = in.static_ptr ? in.static_ptr[g + 1] - s0 : 0;
  const int NC = in.col_ptr[g + 1] - in.col_ptr[g];
  const bool bad_count = N < 1 || N > in.max_lig || N > VD_MAX_LIG || M < 0 || S < 0 || NC < 0 || NC > in.max_col || NC > VD_MAX_COL;
  if (bad_count) {                                          // counts outside the stated maxima: no row of this frame can be placed
    if (tid < 6 && out.totals) out.totals[6 * (size_t)f + tid] = NAN;
    if (tid < 6 && out.totals_fixed) out.totals_fixed[6 * (size_t)f + tid] = VD_BAD_FIXED;
    return;
  }
  const size_t arow = (size_t)(in.lig_pos_off[g] + (long long)k * N);      // the frame's first row of atom_terms (and of lig_pos)
  const size_t crow = (size_t)(in.col_off[g] + (long long)k * NC);         // the frame's first row of col_terms
  const int MR = M + S;
  const Receptor rec = {in.pocket_pos + 3 * (in.pocket_pos_off[g] + (long long)k * M), in.static_pos + 3 * (size_t)s0, nullptr, nullptr, M};
  const int8_t* ptype = in.pocket_type + m0;
  const int8_t* stype = in.static_type + s0;
  const int32_t* pcol = in.pocket_col + m0;
  const int32_t* scol = in.static_col + s0;
  const float cut2 = a.cutoff * a.cutoff;
  int bad_atom = 0;
  FrameBox box;
  {
    const float* lp = in.lig_pos + 3 * arow;
    for (int i = tid; i < N; i += VD_THREADS) {
      const float x = lp[3 * i], y = lp[3 * i + 1], z = lp[3 * i + 2];
      const int t = in.lig_type[l0 + i];
      bad_atom |= !atom_ok(x, y, z);
      lx[i] = make_float4(x, y, z, __int_as_float(v_typed(t) ? t : -1));
      if (v_typed(t)) box.add(x, y, z, 0.f);
    }
  }
  long long* cacc = reinterpret_cast<long long*>(out.col_fixed) + 5 * crow;
  for (int i = tid; i < 5 * NC; i += VD_THREADS) __hip_atomic_store(cacc + i, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  box.block_reduce(redf, lane, wave);                       // its barrier: the ligand complete in LDS, the columns zero
  long long acc[5] = {0, 0, 0, 0, 0};                       // ligand atom tid
  const float4 mine = tid < N ? lx[tid] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
  const bool mine_typed = __float_as_int(mine.w) >= 0;
  int nc = 0;                                               // candidates waiting in the list (uniform)
  for (int b0 = 0; b0 < MR || nc > 0; b0 += VD_THREADS) {
    if (b0 < MR) {                                          // the next receptor tile onto the end of the list
      const int b = b0 + tid;
      bool keep = false;
      float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
      int col = 0;
      if (b < MR) {
        const float* y = rec.pos(b);
        const int t = *rec.sel(b, ptype, stype);
        col = *rec.sel(b, pcol, scol);
        const bool ok = atom_ok(y[0], y[1], y[2]) && col >= 0 && col < NC;
        bad_atom |= !ok;
        c = make_float4(y[0], y[1], y[2], __int_as_float(t));
        keep = ok && v_typed(t) && box.touches(c.x, c.y, c.z, a.cutoff);
      }
      int slot, tot;
      block_compact(keep, nc, wcnt, lane, wave, slot, tot);
      if (keep) { cx[slot] = c; ccol[slot] = col; }         // slot < nc + 256 <= 511
      nc += tot;
      __syncthreads();                                      // the list complete; wcnt free
      if (nc < VD_THREADS && b0 + VD_THREADS < MR) continue;     // not a full tile yet, and more atoms to come
    }
    const int n = min(nc, VD_THREADS);
    if (tid < n) {                                          // columns: a thread per candidate
      const float4 c = cx[tid];
      long long s[5] = {0, 0, 0, 0, 0};
      for (int i = 0; i < N; ++i) {
        const float4 l = lx[i];
        if (__float_as_int(l.w) >= 0) vd_add_pair(l, c, cut2, s);
      }
      long long* dst = cacc + 5 * (size_t)ccol[tid];
#pragma unroll
      for (int q = 0; q < 5; ++q)
        if (s[q]) atomicAdd(reinterpret_cast<unsigned long long*>(dst + q), (unsigned long long)s[q]);
    }
    if (mine_typed)                                         // atoms: a thread per ligand atom
      for (int j = 0; j < n; ++j) vd_add_pair(mine, cx[j], cut2, acc);
    __syncthreads();                                        // the tile is worked off
    if (nc > VD_THREADS) {                                  // the rest moves to the front
      const bool mv = tid < nc - VD_THREADS;
      const float4 c = mv ? cx[VD_THREADS + tid] : make_float4(0.f, 0.f, 0.f, 0.f);
      const int col = mv ? ccol[VD_THREADS + tid] : 0;
      if (mv) { cx[tid] = c; ccol[tid] = col; }
      __syncthreads();
    }
    nc -= n;
  }
  const bool bad = __syncthreads_or(bad_atom);              // uniform; every atomic of the workgroup issued before it
  // per atom
  if (tid < N) {
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      if (out.atom_terms) out.atom_terms[5 * (arow + tid) + q] = bad ? NAN : vd_float(acc[q]);
      if (out.atom_fixed) out.atom_fixed[5 * (arow + tid) + q] = bad ? VD_BAD_FIXED : acc[q];
    }
  }
  // per frame: integer sums over the atoms
#pragma unroll
  for (int q = 0; q < 5; ++q) acc[q] = vd_wave_sum(tid < N ? acc[q] : 0ll);
  if (lane == 0)
    for (int q = 0; q < 5; ++q) redt[wave][q] = acc[q];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's column atomics have reached memory
  __syncthreads();
  if (tid == 0) {
    long long t[6], e = 0;
    for (int q = 0; q < 5; ++q) {
      t[q] = 0;
      for (int w = 0; w < VD_WAVES; ++w) t[q] += redt[w][q];
      e += t[q];
    }
    t[5] = e;
    for (int q = 0; q < 6; ++q) {
      if (out.totals) out.totals[6 * (size_t)f + q] = bad ? NAN : vd_float(t[q]);
      if (out.totals_fixed) out.totals_fixed[6 * (size_t)f + q] = bad ? VD_BAD_FIXED : t[q];
    }
  }
  // per column: the integer sums, read past this CU's L1 (the atomics ran in memory), and their float32 values
  for (int i = tid; i < 5 * NC; i += VD_THREADS) {
    const long long v = __hip_atomic_load(cacc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (out.col_terms) out.col_terms[5 * crow + i] = bad ? NAN : vd_float(v);
    if (bad) cacc[i] = VD_BAD_FIXED;
  }
}

// ------------------------------------------------------------------------------------------------ host
static const char* VD_FN = "dbfr_vina_decompose";

// the host copies of the index arrays, when the caller has them: every count, row offset and column
static int vd_validate(const dbfr_vina_decompose_in& d, const dbfr_vina_decompose_in& h) {
  if (!h.frame_ptr || !h.lig_ptr || !h.lig_pos_off || !h.pocket_ptr || !h.pocket_col || !h.col_ptr || !h.col_off ||
      (d.static_ptr && (!h.static_ptr || !h.static_col)))
    return arg_err(VD_FN, "host: a host copy of an index array is missing");
  const int G = d.n_group;
  if (const int rc = frame_ptr_err(VD_FN, h.frame_ptr, G, d.n_frame)) return rc;
  long long lrow = 0, crow = 0;
  for (int g = 0; g < G; ++g) {
    const std::string where = "group " + std::to_string(g) + ": ";
    const int F = h.frame_ptr[g + 1] - h.frame_ptr[g], N = h.lig_ptr[g + 1] - h.lig_ptr[g], m0 = h.pocket_ptr[g],
              M = h.pocket_ptr[g + 1] - m0, s0 = d.static_ptr ? h.static_ptr[g] : 0, S = d.static_ptr ? h.static_ptr[g + 1] - s0 : 0,
              NC = h.col_ptr[g + 1] - h.col_ptr[g];
    if (const int rc = group_counts_err(VD_FN, where, {{F}, {N, "ligand atoms", "max_lig", d.max_lig}, {M}, {S},
                                                       {NC, "columns", "max_col", d.max_col}}))
      return rc;
    if (N < 1) return arg_err(VD_FN, where + "no ligand atoms");
    if (h.lig_pos_off[g] != lrow) return arg_err(VD_FN, where + "lig_pos_off does not continue the rows of the groups before it");
    if (h.col_off[g] != crow) return arg_err(VD_FN, where + "col_off does not continue the rows of the groups before it");
    lrow += (long long)F * N;
    crow += (long long)F * NC;
    for (int b = 0; b < M + S; ++b) {
      const int col = b < M ? h.pocket_col[m0 + b] : h.static_col[s0 + b - M];
      if (col < 0 || col >= NC) return arg_err(VD_FN, where + "the column of receptor atom " + std::to_string(b) + " is out of range");
    }
  }
  return DBFR_OK;
}

extern "C" int dbfr_vina_decompose(const dbfr_vina_decompose_in* in, const dbfr_vina_decompose_opts* opts,
                                   const dbfr_vina_decompose_out* out, void* hip_stream) {
  const char* fn = VD_FN;
  if (!in || !out) return arg_err(fn, "null argument");
  if (in->n_group < 0 || in->n_frame < 0) return arg_err(fn, "negative n_group / n_frame");
  if (in->max_lig < 0 || in->max_lig > VD_MAX_LIG) return limit_err(fn, "max_lig (ligand atoms)", in->max_lig, 0, VD_MAX_LIG);
  if (in->max_col < 0 || in->max_col > VD_MAX_COL) return limit_err(fn, "max_col (columns)", in->max_col, 0, VD_MAX_COL);
  dbfr_vina_decompose_opts o = {V_CUTOFF};
  if (opts) o = *opts;
  if (!(o.cutoff > 0.f && o.cutoff <= 16.f)) return arg_err(fn, "cutoff must lie in (0, 16] A");
  if (in->n_frame == 0) return DBFR_OK;
  if (in->n_group == 0) return arg_err(fn, "frames without groups");
  if (!in->frame_ptr || !in->lig_ptr || !in->lig_pos_off || !in->lig_pos || !in->lig_type || !in->pocket_ptr || !in->pocket_pos_off ||
      !in->pocket_pos || !in->pocket_type || !in->pocket_col || !in->col_ptr || !in->col_off)
    return arg_err(fn, "frame_ptr / lig_ptr / lig_pos_off / lig_pos / lig_type / pocket_ptr / pocket_pos_off / pocket_pos / pocket_type / "
                       "pocket_col / col_ptr / col_off missing");
  if (in->static_ptr && (!in->static_pos || !in->static_type || !in->static_col))
    return arg_err(fn, "static_ptr given without static_pos / static_type / static_col");
  if (!out->col_fixed) return arg_err(fn, "col_fixed missing: the column sums are accumulated there");
  if (in->host) {
    const int rc = vd_validate(*in, *static_cast<const dbfr_vina_decompose_in*>(in->host));
    if (rc != DBFR_OK) return rc;
  }
  VdArgs a;
  a.in = *in;
  a.in.host = nullptr;
  a.out = *out;
  a.cutoff = o.cutoff;
  HIPCHECK(launch_frames(k_vina_decompose, in->n_frame, VD_THREADS, 0, hip_stream, a));
  return DBFR_OK;
}
