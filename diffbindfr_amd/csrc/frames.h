// The frame-batch layer of the per-pose analysis kernels (posecheck, interactions, pocketcheck, sasa, apoholo, hetero, hydrogens,
// decompose, cavity): one workgroup of 256 threads per frame (one pose of one complex), the frame's group found in frame_ptr,
// CSR-indexed atoms, the receptor = the frame's pocket atoms then the group's static atoms, a bounding box in LDS to reject
// receptor atoms against, survivors compacted in index order by ballot prefixes, and the host-side refusals that go with them.
// Only what the kernels do identically lives here; every float expression of a definition, every filter width and every list
// policy stays in the kernel's own file.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <string>

#include "../../include/dbfr.h"
#include "common.h"

#define FR_THREADS 256
#define FR_WAVES (FR_THREADS / 64)

// ------------------------------------------------------------------------------------------------ device
__device__ __forceinline__ int frame_group(const int32_t* ptr, int n, int x) {   // the last group whose first entry is <= x
  int g = 0, hi = n;
  while (hi - g > 1) {
    const int mid = (g + hi) >> 1;
    if (ptr[mid] <= x) g = mid;
    else hi = mid;
  }
  return g;
}

// reductions over a wave, the result in every lane: minima, maxima and integer sums are exact in any order
__device__ __forceinline__ float wave_min(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// a usable coordinate (finite, within 1e4 A) and a usable radius (in (0, 4] A); NaN fails both
__device__ __forceinline__ bool coord_ok(float v) { return fabsf(v) <= 1e4f; }
__device__ __forceinline__ bool atom_ok(float x, float y, float z) { return coord_ok(x) && coord_ok(y) && coord_ok(z); }
__device__ __forceinline__ bool atom_ok(float x, float y, float z, float r) { return atom_ok(x, y, z) && r > 0.f && r <= 4.f; }

// The bounding box of the atoms a workgroup holds in LDS, with their largest radius.
struct FrameBox {
  float lox = INFINITY, loy = INFINITY, loz = INFINITY, hix = -INFINITY, hiy = -INFINITY, hiz = -INFINITY, rmax = 0.f;
  __device__ __forceinline__ void add(float x, float y, float z, float r) {
    lox = fminf(lox, x); loy = fminf(loy, y); loz = fminf(loz, z);
    hix = fmaxf(hix, x); hiy = fmaxf(hiy, y); hiz = fmaxf(hiz, z);
    rmax = fmaxf(rmax, r);
  }
  // the box of the whole workgroup in every thread, through redf[][0..6]; ONE barrier (whatever else the threads wrote to LDS
  // before the call is complete behind it too)
  __device__ __forceinline__ void block_reduce(float (*redf)[8], int lane, int wave) {
    lox = wave_min(lox); loy = wave_min(loy); loz = wave_min(loz);
    hix = wave_max(hix); hiy = wave_max(hiy); hiz = wave_max(hiz);
    rmax = wave_max(rmax);
    if (lane == 0) {
      redf[wave][0] = lox; redf[wave][1] = loy; redf[wave][2] = loz; redf[wave][3] = hix; redf[wave][4] = hiy; redf[wave][5] = hiz;
      redf[wave][6] = rmax;
    }
    __syncthreads();
    for (int w = 0; w < FR_WAVES; ++w) {
      lox = fminf(lox, redf[w][0]); loy = fminf(loy, redf[w][1]); loz = fminf(loz, redf[w][2]);
      hix = fmaxf(hix, redf[w][3]); hiy = fmaxf(hiy, redf[w][4]); hiz = fmaxf(hiz, redf[w][5]);
      rmax = fmaxf(rmax, redf[w][6]);
    }
  }
  // inside the box grown by `grow` on every side (the kernel's own expression: it is the width of its filter)
  __device__ __forceinline__ bool touches(float x, float y, float z, float grow) const {
    return x >= lox - grow && x <= hix + grow && y >= loy - grow && y <= hiy + grow && z >= loz - grow && z <= hiz + grow;
  }
};

// One tile of a compaction in index order: thread t of the workgroup holds candidate flag c; `slot` = base + the candidates of the
// threads before it, `total` = the candidates of the tile (uniform).  ONE barrier, behind the write of wcnt.  The caller stores
// at `slot` -- or drops the entry, works the list off first, or goes to memory when it is full: that policy is the kernel's -- and
// then issues the __syncthreads() that completes the entries and frees wcnt for the next tile.
__device__ __forceinline__ void block_compact(bool c, int base, int* wcnt, int lane, int wave, int& slot, int& total) {
  const unsigned long long bal = __ballot(c);
  const int pre = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wcnt[wave] = __popcll(bal);
  __syncthreads();
  int off = base, tot = 0;
  for (int w = 0; w < FR_WAVES; ++w) {
    off += w < wave ? wcnt[w] : 0;
    tot += wcnt[w];
  }
  slot = off + pre;
  total = tot;
}

// The receptor of a frame: atom b < M is pocket atom b of the frame, atom b >= M static atom b - M of the group.  `pp` / `sp`
// are the frame's and the group's first position; the per-atom arrays of a kernel go through sel() with the group's base added.
struct Receptor {
  const float *pp, *sp;
  const float *prad, *srad;          // radii, where the kernel reads them (else nullptr)
  int M;
  template <class T>
  __device__ __forceinline__ const T* sel(int b, const T* pocket, const T* stat, int stride = 1) const {
    return b < M ? pocket + stride * (size_t)b : stat + stride * (size_t)(b - M);
  }
  __device__ __forceinline__ const float* pos(int b) const { return sel(b, pp, sp, 3); }
  __device__ __forceinline__ float rad(int b) const { return *sel(b, prad, srad); }
};

// ------------------------------------------------------------------------------------------------ host
static inline int arg_err(const char* fn, const std::string& text) {
  dbfr_set_error(std::string(fn) + ": " + text);
  return DBFR_ERR_ARG;
}

static inline int limit_err(const char* fn, const char* what, long long got, int lo, int hi) {
  return arg_err(fn, std::string(what) + " " + std::to_string(got) + " outside [" + std::to_string(lo) + ", " + std::to_string(hi) +
                         "]: groups beyond it are not supported");
}

// The counts of the host copies: frame_ptr runs from 0 to n_frame; per group no count is negative and none exceeds the maximum
// the caller stated for it (what == nullptr: none stated).
static inline int frame_ptr_err(const char* fn, const int32_t* frame_ptr, int n_group, int n_frame) {
  return frame_ptr[0] != 0 || frame_ptr[n_group] != n_frame ? arg_err(fn, "frame_ptr does not run from 0 to n_frame") : DBFR_OK;
}
struct GroupCount {
  long long n;
  const char *what, *max_name;
  long long max;
};
static inline int group_counts_err(const char* fn, const std::string& where, std::initializer_list<GroupCount> counts) {
  for (const GroupCount& c : counts)
    if (c.n < 0) return arg_err(fn, where + "a negative count");
  for (const GroupCount& c : counts)
    if (c.what && c.n > c.max)
      return arg_err(fn, where + std::to_string(c.n) + " " + c.what + ", " + c.max_name + " says " + std::to_string(c.max));
  return DBFR_OK;
}

// Every receptor atom of a group (pocket, then static): the radius in (0, 4], the residue column in [0, NR); between(b) runs
// between the two and refuses what else the kernel reads of atom b.
template <class Between>
static inline int receptor_atoms_err(const char* fn, const std::string& where, int M, int S, const float* prad, const float* srad,
                                     const int32_t* pcol, const int32_t* scol, int NR, Between between) {
  for (int b = 0; b < M + S; ++b) {
    const float r = b < M ? prad[b] : srad[b - M];
    const int col = b < M ? pcol[b] : scol[b - M];
    if (!(r > 0.f && r <= 4.f)) return arg_err(fn, where + "the radius of receptor atom " + std::to_string(b) + " lies outside (0, 4]");
    if (const int rc = between(b)) return rc;
    if (col < 0 || col >= NR) return arg_err(fn, where + "the residue column of receptor atom " + std::to_string(b) + " is out of range");
  }
  return DBFR_OK;
}

// One workgroup per frame on `stream`; dynamic LDS above 32 KB is asked for first.  Returns the launch's status.
template <class Kernel, class Args>
static inline hipError_t launch_frames(Kernel kernel, int n_frame, int threads, size_t lds, void* stream, const Args& a) {
  if (lds > 32 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_frame), dim3((unsigned)threads), lds, (hipStream_t)stream, a);
  return hipGetLastError();
}
