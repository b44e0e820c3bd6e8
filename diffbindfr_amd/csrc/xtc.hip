// XTC trajectory encoding on the device: the frames the sampler keeps in HBM (ligand + pocket atom14 per (pose, frame)) turned
// into the bytes libxdrfile's xdrfile_compress_coord_float (GROMACS xdr3dfcoord) writes for the coordinates a reader gets back
// from the frame PDB files.  include/dbfr.h states the interface, docs/trajectory.md the coordinate chain and the format.
//
// Four launches on the caller's stream:
//   k_xtc_quant   one workgroup per frame: gather through the atom map, the PDB / nm / precision chain, the int32 triples into
//                 the workspace; minint / maxint and the smallest |dx|+|dy|+|dz| of consecutive atoms by block reduction
//                 (integer min / max only).
//   k_xtc_pack    one wave per frame: the sequential run-length walk.  The wave stages a window of the frame's triples in LDS
//                 and every lane walks it in lockstep (uniform control flow, broadcast LDS reads); lane 0 stores the header
//                 and the bit stream, as big-endian dwords, into the frame's worst-case slot.
//   k_xtc_scan    one workgroup: checks the frame -> file table, exclusive scan of the frame byte counts, the file offsets and
//                 the refusal status.
//   k_xtc_concat  one workgroup per frame: dword copy of the frame's bytes to its place in the file images.
// A frame's bytes depend on that frame alone (no cross-frame reduction, no atomics); no scratch (resource report in profiles/).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <string>

#include "../../include/dbfr.h"
#include "common.h"

#define XQ_THREADS 256
#define XP_WIN 2048                  // atoms of a frame staged in LDS by k_xtc_pack (24 KB)
#define XP_KEEP 16                   // atoms behind the walk kept when the window moves (a run reaches 8 back)
#define XS_THREADS 1024
#define XTC_FIRSTIDX 9
#define XTC_LASTIDX 73
#define XTC_MAXABS (INT_MAX - 2)
#define XTC_MAX_FRAMES (1 << 20)
#define XTC_MAX_ATOMS (1 << 20)
#define XTC_MM 12                    // ints per frame: minint[3], maxint[3], mindiff, error bits, natoms
#define XTC_HDR_WORDS 14             // 1995, natoms, step, time, box[9], natoms
#define XTC_CHDR_WORDS 9             // precision, minint[3], maxint[3], smallidx, nbytes

// error bits (the status word)
#define XE_OVERFLOW 1
#define XE_TABLE 2
#define XE_INDEX 4
#define XE_ORDER 8
#define XE_CAP 16

__constant__ int kMagic[XTC_LASTIDX] = {
    0, 0, 0, 0, 0, 0, 0, 0, 0, 8, 10, 12, 16, 20, 25, 32, 40, 50, 64, 80, 101, 128, 161, 203, 256, 322, 406, 512, 645, 812,
    1024, 1290, 1625, 2048, 2580, 3250, 4096, 5060, 6501, 8192, 10321, 13003, 16384, 20642, 26007, 32768, 41285, 52015,
    65536, 82570, 104031, 131072, 165140, 208063, 262144, 330280, 416127, 524287, 660561, 832255, 1048576, 1321122,
    1664510, 2097152, 2642245, 3329021, 4194304, 5284491, 6658042, 8388607, 10568983, 13316085, 16777216};

struct XtcArgs {
  dbfr_xtc_in in;
  dbfr_xtc_opts o;
  int32_t* q;                        // [n_frame, max_atoms, 3]
  uint8_t* slots;                    // [n_frame, slot_bytes]
  int64_t slot_bytes;
  int32_t* mm;                       // [n_frame, XTC_MM]
  int32_t* fsize;                    // [n_frame]
  int64_t* foff;                     // [n_frame + 1]
  int32_t* status;
  uint8_t* out;
  int64_t out_cap;
  int64_t* offsets;                  // [n_file + 1]
};

static int64_t xtc_slot_bytes(int max_atoms) { return ((16LL * max_atoms + 256) + 15) & ~15LL; }

__device__ __forceinline__ uint32_t be32(uint32_t v) { return __builtin_bswap32(v); }

// the frame's atom map: natoms (0 on an error) and its first entry; error bits in err
__device__ __forceinline__ int frame_map(const dbfr_xtc_in& in, int f, int& m0, int& src, int& err) {
  const int file = in.frame_file[f];
  src = in.frame_src[f];
  m0 = 0;
  if (file < 0 || file >= in.n_file || src < 0 || src >= in.n_src) { err |= XE_INDEX; return 0; }
  const int m = in.file_map[file];
  if (m < 0 || m >= in.n_map) { err |= XE_INDEX; return 0; }
  m0 = in.map_ptr[m];
  const int n = in.map_ptr[m + 1] - m0;
  if (m0 < 0 || n < 1 || n > in.max_atoms || m0 + n > in.map_ptr[in.n_map] || in.map_ptr[in.n_map] < 0) { err |= XE_INDEX; return 0; }
  return n;
}

__device__ __forceinline__ int wave_min(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_or(int v) {
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(XQ_THREADS) void k_xtc_quant(XtcArgs a) {
  __shared__ int s[XQ_THREADS + 1][3];           // s[t + 1] = triple of this pass's atom t, s[0] = the previous pass's last
  __shared__ int red[XQ_THREADS / 64][8];
  const dbfr_xtc_in& in = a.in;
  const int f = blockIdx.x, tid = threadIdx.x;
  int err = 0, m0, src;
  const int natoms = frame_map(in, f, m0, src, err);
  const bool raw = natoms <= 9;                  // stored uncompressed: the ints hold the bits of the nm floats
  const float prec = a.o.precision;
  const float cx = in.center[0], cy = in.center[1], cz = in.center[2];
  int32_t* q = a.q + (size_t)f * in.max_atoms * 3;
  int mn0 = INT_MAX, mn1 = INT_MAX, mn2 = INT_MAX, mx0 = INT_MIN, mx1 = INT_MIN, mx2 = INT_MIN, mdiff = INT_MAX;
  for (int base = 0; base < natoms; base += XQ_THREADS) {
    __syncthreads();
    if (tid < 3) s[0][tid] = s[XQ_THREADS][tid];
    __syncthreads();
    const int k = base + tid;
    if (k < natoms) {
      const int code = in.atom_map[m0 + k];
      float x[3] = {0.f, 0.f, 0.f};
      if (code < 0) {
        const int m = -1 - code;
        if (m < in.n_static) { const float* p = in.static_pos + (size_t)m * 3; x[0] = p[0]; x[1] = p[1]; x[2] = p[2]; }
        else err |= XE_INDEX;
      } else if (code >= 0x40000000) {
        const int rs = code - 0x40000000;
        if (rs < in.n_res * 14) {
          const float* p = in.pos14 + ((size_t)src * in.n_res * 14 + rs) * 3;
          x[0] = p[0] + cx; x[1] = p[1] + cy; x[2] = p[2] + cz;
        } else err |= XE_INDEX;
      } else {
        if (code < in.n_lig) {
          const float* p = in.lig + ((size_t)src * in.n_lig + code) * 3;
          x[0] = p[0] + cx; x[1] = p[1] + cy; x[2] = p[2] + cz;
        } else err |= XE_INDEX;
      }
      int l[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double q3 = rint((double)x[c] * 1000.0);          // "%8.3f": the exact value rounded, ties to even
        const float xp = (float)(q3 / 1000.0);                   // what a PDB reader stores
        const float xn = xp * 0.1f;                              // A -> nm
        if (raw) {
          l[c] = __float_as_int(xn);
        } else {
          const float p = xn * prec;
          const float lf = xn >= 0.f ? (float)((double)p + 0.5) : (float)((double)p - 0.5);
          if (!(fabs((double)lf) <= (double)XTC_MAXABS)) { err |= XE_OVERFLOW; l[c] = 0; }
          else l[c] = (int)lf;
        }
        q[(size_t)k * 3 + c] = l[c];
        s[tid + 1][c] = l[c];
      }
      mn0 = min(mn0, l[0]); mn1 = min(mn1, l[1]); mn2 = min(mn2, l[2]);
      mx0 = max(mx0, l[0]); mx1 = max(mx1, l[1]); mx2 = max(mx2, l[2]);
    }
    __syncthreads();
    if (!raw && k < natoms && k >= 1) {
      const long long d = llabs((long long)s[tid + 1][0] - s[tid][0]) + llabs((long long)s[tid + 1][1] - s[tid][1]) +
                          llabs((long long)s[tid + 1][2] - s[tid][2]);
      mdiff = min(mdiff, (int)min(d, (long long)INT_MAX));
    }
  }
  mn0 = wave_min(mn0); mn1 = wave_min(mn1); mn2 = wave_min(mn2);
  mx0 = wave_max(mx0); mx1 = wave_max(mx1); mx2 = wave_max(mx2);
  mdiff = wave_min(mdiff);
  err = wave_or(err);
  const int w = tid >> 6;
  if ((tid & 63) == 0) {
    red[w][0] = mn0; red[w][1] = mn1; red[w][2] = mn2; red[w][3] = mx0; red[w][4] = mx1; red[w][5] = mx2;
    red[w][6] = mdiff; red[w][7] = err;
  }
  __syncthreads();
  if (tid < 8) {
    int v = red[0][tid];
    for (int u = 1; u < XQ_THREADS / 64; ++u) {
      const int o = red[u][tid];
      v = tid < 3 || tid == 6 ? min(v, o) : (tid < 6 ? max(v, o) : (v | o));
    }
    red[0][tid] = v;
  }
  __syncthreads();
  if (tid < 7) a.mm[(size_t)f * XTC_MM + tid] = red[0][tid];
  if (tid == 7) {
    int e = red[0][7];
    if (!raw && natoms > 0)                     // the range check of the reference (float arithmetic)
      for (int c = 0; c < 3; ++c)
        if ((float)red[0][3 + c] - (float)red[0][c] >= (float)XTC_MAXABS) e |= XE_OVERFLOW;
    a.mm[(size_t)f * XTC_MM + 7] = e;
  }
  if (tid == 8) a.mm[(size_t)f * XTC_MM + 8] = natoms;
}

// ------------------------------------------------------------------------------------------------ k_xtc_pack
// MSB-first bit stream into big-endian dwords (the bytes of libxdrfile's sendbits, zero-padded to a multiple of 4)
struct BitOut {
  uint32_t* out;
  int cap;                           // dwords available
  int nw;
  int nacc;
  uint64_t acc;
  bool store;                        // lane 0
  bool full;
  __device__ __forceinline__ void put(int n, uint32_t v) {            // n <= 32
    if (n <= 0) return;
    const uint64_t m = n == 32 ? 0xffffffffull : ((1ull << n) - 1);
    acc = (acc << n) | ((uint64_t)v & m);
    nacc += n;
    if (nacc >= 32) {
      nacc -= 32;
      if (nw < cap) { if (store) out[nw] = be32((uint32_t)(acc >> nacc)); ++nw; }
      else full = true;
    }
  }
  __device__ __forceinline__ void zeros(int n) {
    while (n > 0) { const int k = min(n, 32); put(k, 0u); n -= k; }
  }
  __device__ __forceinline__ void flush() {
    if (nacc > 0) {
      if (nw < cap) { if (store) out[nw] = be32((uint32_t)(acc << (32 - nacc))); ++nw; }
      else full = true;
    }
  }
  __device__ __forceinline__ int64_t bits() const { return (int64_t)(nw - (nacc > 0 ? 1 : 0)) * 32 + nacc; }
};

// bit length of v (libxdrfile sizeofint for v >= 1)
__device__ __forceinline__ int bitlen64(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

// value = (n0 * s1 + n1) * s2 + n2 (n0, n1, n2 < 2^24, s1, s2 <= 2^24): hi * 2^32 + lo
__device__ __forceinline__ void mixed3(uint32_t n0, uint32_t n1, uint32_t n2, uint32_t s1, uint32_t s2, uint64_t& hi, uint64_t& lo) {
  const uint64_t v = (uint64_t)n0 * s1 + n1;
  lo = (v & 0xffffffffull) * s2 + n2;
  hi = (v >> 32) * s2 + (lo >> 32);
  lo &= 0xffffffffull;
}

// libxdrfile sizeofints(3, sizes): the bit length of sizes[0] * sizes[1] * sizes[2]
__device__ __forceinline__ int sizeofints3(uint32_t s0, uint32_t s1, uint32_t s2) {
  uint64_t hi, lo;
  mixed3(s0, 0, 0, s1, s2, hi, lo);
  return hi ? 32 + bitlen64(hi) : max(bitlen64(lo), 0);
}

// libxdrfile sendints(buf, 3, nbits, sizes, nums): the mixed-radix number as its nb little-endian bytes (nb >= 1)
__device__ __forceinline__ void sendints3(BitOut& bo, int nbits, uint32_t s1, uint32_t s2, uint32_t n0, uint32_t n1, uint32_t n2) {
  uint64_t hi, lo;
  mixed3(n0, n1, n2, s1, s2, hi, lo);
  const int nb = hi ? 4 + (bitlen64(hi) + 7) / 8 : max(1, (bitlen64(lo) + 7) / 8);
  const uint64_t bytes_lo = lo, bytes_hi = hi;
  if (nbits >= nb * 8) {
    for (int k = 0; k < nb; ++k) bo.put(8, (uint32_t)((k < 4 ? bytes_lo >> (8 * k) : bytes_hi >> (8 * (k - 4))) & 0xff));
    bo.zeros(nbits - nb * 8);
  } else {
    for (int k = 0; k < nb - 1; ++k) bo.put(8, (uint32_t)((k < 4 ? bytes_lo >> (8 * k) : bytes_hi >> (8 * (k - 4))) & 0xff));
    const int k = nb - 1;
    bo.put(nbits - 8 * k, (uint32_t)((k < 4 ? bytes_lo >> (8 * k) : bytes_hi >> (8 * (k - 4))) & 0xff));
  }
}

__global__ __launch_bounds__(64) void k_xtc_pack(XtcArgs a) {
  __shared__ int w[XP_WIN * 3];
  const dbfr_xtc_in& in = a.in;
  const int f = blockIdx.x, lane = threadIdx.x;
  const int32_t* mmf = a.mm + (size_t)f * XTC_MM;
  int err = mmf[7];
  const int natoms = mmf[8];
  uint32_t* slot = reinterpret_cast<uint32_t*>(a.slots + (size_t)f * a.slot_bytes);
  const int32_t* q = a.q + (size_t)f * in.max_atoms * 3;
  if (err || natoms < 1) {
    if (lane == 0) a.fsize[f] = 0;
    return;
  }
  const int step = a.o.first_step + in.frame_step[f];
  const float time = (float)((double)step * (double)a.o.dt);
  if (lane == 0) {
    slot[0] = be32(1995u); slot[1] = be32((uint32_t)natoms); slot[2] = be32((uint32_t)step); slot[3] = be32(__float_as_uint(time));
    for (int c = 0; c < 9; ++c) slot[4 + c] = be32(__float_as_uint(a.o.box[c]));
    slot[13] = be32((uint32_t)natoms);
  }
  if (natoms <= 9) {                                          // uncompressed nm floats
    if (lane < 3 * natoms) slot[XTC_HDR_WORDS + lane] = be32((uint32_t)q[lane]);
    if (lane == 0) a.fsize[f] = 4 * (XTC_HDR_WORDS + 3 * natoms);
    return;
  }
  const int minint[3] = {mmf[0], mmf[1], mmf[2]};
  const int maxint[3] = {mmf[3], mmf[4], mmf[5]};
  const int mindiff = mmf[6];
  uint32_t sizeint[3];
  int bitsizeint[3] = {0, 0, 0};
  for (int c = 0; c < 3; ++c) sizeint[c] = (uint32_t)maxint[c] - (uint32_t)minint[c] + 1u;
  int bitsize;
  if ((sizeint[0] | sizeint[1] | sizeint[2]) > 0xffffffu) {
    for (int c = 0; c < 3; ++c) bitsizeint[c] = bitlen64(sizeint[c]);
    bitsize = 0;
  } else {
    bitsize = sizeofints3(sizeint[0], sizeint[1], sizeint[2]);
  }
  int smallidx = XTC_FIRSTIDX;
  while (smallidx < XTC_LASTIDX && kMagic[smallidx] < mindiff) ++smallidx;
  if (smallidx + 8 >= XTC_LASTIDX) {                          // the reference would read past its table: refused
    if (lane == 0) { a.fsize[f] = 0; a.mm[(size_t)f * XTC_MM + 7] = XE_TABLE; }
    return;
  }
  const int maxidx = min(XTC_LASTIDX, smallidx + 8), minidx = maxidx - 8;
  int smaller = kMagic[max(XTC_FIRSTIDX, smallidx - 1)] / 2;
  int smallnum = kMagic[smallidx] / 2;
  uint32_t sizesmall = (uint32_t)kMagic[smallidx];
  const int larger = kMagic[maxidx] / 2;
  const int smallidx0 = smallidx;

  BitOut bo{slot + XTC_HDR_WORDS + XTC_CHDR_WORDS, (int)(a.slot_bytes / 4) - XTC_HDR_WORDS - XTC_CHDR_WORDS, 0, 0, 0ull, lane == 0, false};
  // LDS window [wbase, wend) of the frame's triples; every lane runs the same walk
  int wbase = 0, wend = min(natoms, XP_WIN);
  for (int t = lane; t < wend * 3; t += 64) w[t] = q[t];
  __syncthreads();
  auto ensure = [&](int j) {                                  // atom j (>= wbase) in the window; uniform over the wave
    if (j < wend) return;
    const int nb = j - XP_KEEP;
    const int keep = wend - nb;                               // modified atoms behind the walk move with the window
    int v = 0;
    if (lane < keep * 3) v = w[(nb - wbase) * 3 + lane];
    __syncthreads();
    if (lane < keep * 3) w[lane] = v;
    const int ne = min(natoms, nb + XP_WIN);
    for (int t = keep * 3 + lane; t < (ne - nb) * 3; t += 64) w[t] = q[(size_t)nb * 3 + t];
    __syncthreads();
    wbase = nb;
    wend = ne;
  };
  auto at = [&](int j, int c) -> int& { return w[(j - wbase) * 3 + c]; };

  int prevrun = -1, prev0 = 0, prev1 = 0, prev2 = 0;
  int i = 0;
  while (i < natoms) {
    int is_small = 0, is_smaller;
    ensure(i);
    if (smallidx < maxidx && i >= 1 && abs(at(i, 0) - prev0) < larger && abs(at(i, 1) - prev1) < larger &&
        abs(at(i, 2) - prev2) < larger)
      is_smaller = 1;
    else if (smallidx > minidx)
      is_smaller = -1;
    else
      is_smaller = 0;
    if (i + 1 < natoms) {
      ensure(i + 1);
      if (abs(at(i, 0) - at(i + 1, 0)) < smallnum && abs(at(i, 1) - at(i + 1, 1)) < smallnum &&
          abs(at(i, 2) - at(i + 1, 2)) < smallnum) {
        // interchange the first with the second atom (better compression of water molecules)
        for (int c = 0; c < 3; ++c) {
          const int t0 = at(i, c), t1 = at(i + 1, c);
          __syncthreads();
          at(i, c) = t1;
          at(i + 1, c) = t0;
        }
        __syncthreads();
        is_small = 1;
      }
    }
    const uint32_t t0 = (uint32_t)at(i, 0) - (uint32_t)minint[0], t1 = (uint32_t)at(i, 1) - (uint32_t)minint[1],
                   t2 = (uint32_t)at(i, 2) - (uint32_t)minint[2];
    if (bitsize == 0) {
      bo.put(bitsizeint[0], t0);
      bo.put(bitsizeint[1], t1);
      bo.put(bitsizeint[2], t2);
    } else {
      sendints3(bo, bitsize, sizeint[1], sizeint[2], t0, t1, t2);
    }
    prev0 = at(i, 0); prev1 = at(i, 1); prev2 = at(i, 2);
    ++i;
    int run = 0;
    if (is_small == 0 && is_smaller == -1) is_smaller = 0;
    const int rs = i, rp0 = prev0, rp1 = prev1, rp2 = prev2;     // the run's atoms are sent after the run-length flag
    while (is_small && run < 8 * 3) {
      const int d0 = at(i, 0) - prev0, d1 = at(i, 1) - prev1, d2 = at(i, 2) - prev2;
      const int tmpsum = (int)((uint32_t)d0 * (uint32_t)d0 + (uint32_t)d1 * (uint32_t)d1 + (uint32_t)d2 * (uint32_t)d2);
      if (is_smaller == -1 && tmpsum >= (int)((uint32_t)smaller * (uint32_t)smaller)) is_smaller = 0;
      run += 3;
      prev0 = at(i, 0); prev1 = at(i, 1); prev2 = at(i, 2);
      ++i;
      is_small = 0;
      if (i < natoms) {
        ensure(i);
        if (abs(at(i, 0) - prev0) < smallnum && abs(at(i, 1) - prev1) < smallnum && abs(at(i, 2) - prev2) < smallnum) is_small = 1;
      }
    }
    if (run != prevrun || is_smaller != 0) {
      prevrun = run;
      bo.put(1, 1u);
      bo.put(5, (uint32_t)(run + is_smaller + 1));
    } else {
      bo.put(1, 0u);
    }
    int p0 = rp0, p1 = rp1, p2 = rp2;
    for (int k = 0; k < run / 3; ++k) {
      const int c0 = at(rs + k, 0), c1 = at(rs + k, 1), c2 = at(rs + k, 2);
      sendints3(bo, smallidx, sizesmall, sizesmall, (uint32_t)(c0 - p0 + smallnum), (uint32_t)(c1 - p1 + smallnum),
                (uint32_t)(c2 - p2 + smallnum));
      p0 = c0; p1 = c1; p2 = c2;
    }
    if (is_smaller != 0) {
      smallidx += is_smaller;
      if (is_smaller < 0) {
        smallnum = smaller;
        smaller = kMagic[smallidx - 1] / 2;
      } else {
        smaller = smallnum;
        smallnum = kMagic[smallidx] / 2;
      }
      sizesmall = (uint32_t)kMagic[smallidx];
    }
  }
  bo.flush();
  const int64_t nbytes = (bo.bits() + 7) / 8;
  if (lane == 0) {
    uint32_t* h = slot + XTC_HDR_WORDS;
    h[0] = be32(__float_as_uint(a.o.precision));
    for (int c = 0; c < 3; ++c) { h[1 + c] = be32((uint32_t)minint[c]); h[4 + c] = be32((uint32_t)maxint[c]); }
    h[7] = be32((uint32_t)smallidx0);
    h[8] = be32((uint32_t)nbytes);
    if (bo.full) { a.fsize[f] = 0; a.mm[(size_t)f * XTC_MM + 7] = XE_CAP; }
    else a.fsize[f] = 4 * (XTC_HDR_WORDS + XTC_CHDR_WORDS + bo.nw);
  }
}

// ------------------------------------------------------------------------------------------------ scan + concat
__global__ __launch_bounds__(XS_THREADS) void k_xtc_scan(XtcArgs a) {
  __shared__ long long wsum[XS_THREADS / 64];
  __shared__ int werr[XS_THREADS / 64];
  const dbfr_xtc_in& in = a.in;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  long long carry = 0;
  int err = 0;
  for (int base = 0; base < in.n_frame; base += XS_THREADS) {
    const int f = base + tid;
    long long v = 0;
    if (f < in.n_frame) {
      v = a.fsize[f];
      err |= a.mm[(size_t)f * XTC_MM + 7];
      const int ff = in.frame_file[f], pf = f ? in.frame_file[f - 1] : -1;
      if (!(ff == pf || ff == pf + 1) || ff < 0 || ff >= in.n_file) err |= XE_ORDER;
      if (f == in.n_frame - 1 && ff != in.n_file - 1) err |= XE_ORDER;
    }
    long long x = v;                                        // inclusive wave scan
    for (int o = 1; o < 64; o <<= 1) {
      const long long y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    __syncthreads();
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    long long before = carry;
    for (int u = 0; u < wv; ++u) before += wsum[u];
    long long total = carry;
    for (int u = 0; u < XS_THREADS / 64; ++u) total += wsum[u];
    if (f < in.n_frame) {
      const long long off = before + x - v;
      a.foff[f] = off;
      const int ff = in.frame_file[f];
      if (ff >= 0 && ff < in.n_file && (f == 0 || in.frame_file[f - 1] != ff)) a.offsets[ff] = off;
    }
    carry = total;
  }
  err = wave_or(err);
  if (lane == 0) werr[wv] = err;
  __syncthreads();
  if (tid == 0) {
    int e = 0;
    for (int u = 0; u < XS_THREADS / 64; ++u) e |= werr[u];
    if (carry > a.out_cap) e |= XE_CAP;
    a.foff[in.n_frame] = carry;
    a.offsets[in.n_file] = carry;
    a.status[0] = e;
  }
}

__global__ __launch_bounds__(256) void k_xtc_concat(XtcArgs a) {
  if (a.status[0]) return;
  const int f = blockIdx.x;
  const int n = a.fsize[f] >> 2;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.slots + (size_t)f * a.slot_bytes);
  uint32_t* dst = reinterpret_cast<uint32_t*>(a.out + a.foff[f]);
  for (int t = threadIdx.x; t < n; t += 256) dst[t] = src[t];
}

// ------------------------------------------------------------------------------------------------ host entry points
static int xtc_check(const dbfr_xtc_in* in) {
  if (!in) { dbfr_set_error("null argument"); return DBFR_ERR_ARG; }
  if (in->n_frame < 1 || in->n_frame > XTC_MAX_FRAMES) { dbfr_set_error("n_frame outside [1, 2^20]"); return DBFR_ERR_ARG; }
  if (in->n_file < 1 || in->n_file > in->n_frame) { dbfr_set_error("n_file outside [1, n_frame]"); return DBFR_ERR_ARG; }
  if (in->max_atoms < 1 || in->max_atoms > XTC_MAX_ATOMS) { dbfr_set_error("max_atoms outside [1, 2^20]"); return DBFR_ERR_ARG; }
  if (in->n_src < 1 || in->n_lig < 0 || in->n_res < 0 || in->n_static < 0 || in->n_map < 1 || in->n_res > (1 << 24) / 14) {
    dbfr_set_error("bad sizes (n_src >= 1, n_map >= 1, n_lig / n_res / n_static >= 0)");
    return DBFR_ERR_ARG;
  }
  if ((in->n_lig && !in->lig) || (in->n_res && !in->pos14) || (in->n_static && !in->static_pos) || !in->center || !in->map_ptr ||
      !in->atom_map || !in->file_map || !in->frame_file || !in->frame_src || !in->frame_step) {
    dbfr_set_error("null table");
    return DBFR_ERR_ARG;
  }
  return DBFR_OK;
}

struct XtcLayout {
  size_t q, slots, mm, fsize, foff, status, total;
  int64_t slot_bytes, out_cap;
};

static XtcLayout xtc_layout(const dbfr_xtc_in* in) {
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  XtcLayout L;
  L.slot_bytes = xtc_slot_bytes(in->max_atoms);
  size_t o = 0;
  L.q = o; o += al((size_t)in->n_frame * in->max_atoms * 3 * 4);
  L.slots = o; o += al((size_t)in->n_frame * L.slot_bytes);
  L.mm = o; o += al((size_t)in->n_frame * XTC_MM * 4);
  L.fsize = o; o += al((size_t)in->n_frame * 4);
  L.foff = o; o += al(((size_t)in->n_frame + 1) * 8);
  L.status = o; o += 256;
  L.total = o;
  L.out_cap = (int64_t)in->n_frame * L.slot_bytes;
  return L;
}

extern "C" int dbfr_xtc_workspace_bytes(const dbfr_xtc_in* in, size_t* bytes, int64_t* out_cap) {
  int rc = xtc_check(in);
  if (rc) return rc;
  XtcLayout L = xtc_layout(in);
  if (bytes) *bytes = L.total;
  if (out_cap) *out_cap = L.out_cap;
  return DBFR_OK;
}

extern "C" int dbfr_xtc_encode(const dbfr_xtc_in* in, const dbfr_xtc_opts* opts, uint8_t* out, int64_t out_cap, int64_t* offsets,
                               void* workspace, size_t workspace_bytes, void* hip_stream) {
  int rc = xtc_check(in);
  if (rc) return rc;
  XtcLayout L = xtc_layout(in);
  if (!workspace || workspace_bytes < L.total || ((uintptr_t)workspace & 255)) {
    dbfr_set_error("workspace missing, too small or not 256-byte aligned (dbfr_xtc_workspace_bytes)");
    return DBFR_ERR_ARG;
  }
  if (!out || !offsets || out_cap < 0 || ((uintptr_t)out & 3)) { dbfr_set_error("out / offsets missing or out not 4-byte aligned"); return DBFR_ERR_ARG; }
  XtcArgs a;
  a.in = *in;
  a.o.precision = 1000.f;
  a.o.dt = 1.f;
  a.o.first_step = 0;
  for (int c = 0; c < 9; ++c) a.o.box[c] = 0.f;
  if (opts) {
    a.o = *opts;
    if (!(a.o.precision > 0.f)) a.o.precision = 1000.f;             // libxdrfile: precision <= 0 -> 1000
    if (!std::isfinite(a.o.precision) || !std::isfinite(a.o.dt)) { dbfr_set_error("precision / dt not finite"); return DBFR_ERR_ARG; }
  }
  uint8_t* ws = (uint8_t*)workspace;
  a.q = (int32_t*)(ws + L.q);
  a.slots = ws + L.slots;
  a.slot_bytes = L.slot_bytes;
  a.mm = (int32_t*)(ws + L.mm);
  a.fsize = (int32_t*)(ws + L.fsize);
  a.foff = (int64_t*)(ws + L.foff);
  a.status = (int32_t*)(ws + L.status);
  a.out = out;
  a.out_cap = out_cap;
  a.offsets = offsets;
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(k_xtc_quant, dim3(in->n_frame), dim3(XQ_THREADS), 0, st, a);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(k_xtc_pack, dim3(in->n_frame), dim3(64), 0, st, a);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(k_xtc_scan, dim3(1), dim3(XS_THREADS), 0, st, a);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(k_xtc_concat, dim3(in->n_frame), dim3(256), 0, st, a);
  HIPCHECK(hipGetLastError());
  int32_t status = 0;
  HIPCHECK(hipMemcpyAsync(&status, a.status, sizeof status, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  if (status) {
    std::string m = "dbfr_xtc_encode refused the batch:";
    if (status & XE_OVERFLOW) m += " coordinate overflow (|x * precision| beyond INT_MAX - 2 or the range too wide);";
    if (status & XE_TABLE) m += " consecutive atoms too far apart for the XTC table (smallidx + 8 >= 73);";
    if (status & XE_INDEX) m += " an index outside its array (atom map, source frame, file map) or a map longer than max_atoms;";
    if (status & XE_ORDER) m += " frame_file is not 0, 1, ..., n_file - 1 in frame order;";
    if (status & XE_CAP) m += " output larger than out_cap;";
    dbfr_set_error(m);
    return DBFR_ERR_ARG;
  }
  return DBFR_OK;
}
