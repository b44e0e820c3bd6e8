// Protein-ligand interaction fingerprints of poses: one 16-bit word per (frame, residue) and per-kind residue counts for every
// frame of a ragged batch, in one launch.  include/dbfr.h states the definitions; docs/interactions.md the layout and the limits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/dbfr.h"
#include "common.h"
#include "frames.h"

// One workgroup per frame.  The ligand (positions, XS types, neighbour lists) and the centres and normals of its groups in this
// frame are staged in LDS next to one 16-bit word per residue (two to a 32-bit LDS word).  The receptor atoms (pocket atoms of
// the frame, then the static atoms of the group) stream past one per thread against the ligand atoms in LDS: a distance
// early-out first, the receptor atom's bonded neighbours fetched from memory only on a hit.  The receptor groups then stream
// past one per thread: centre and normal from this frame's positions, tested against the ligand groups.  Hits are ORed into the
// LDS words with integer atomics; the row is written coalesced and the per-kind counts are popcounts of ballots.  Only integer
// ORs and sums leave a thread: the bits of a frame do not depend on the launch it is part of.
#define IF_THREADS FR_THREADS
#define IF_MAX_LIG 256
#define IF_MAX_LGRP 32
#define IF_MAX_RES 16384
#define IF_GROUP_W 6               // atoms per group (-1 padded)
#define IF_KINDS 10
#define IF_EARLY 0.001f            // A: the early-out is wider than the widest atom-pair threshold by this much

// XS type classes as bit sets over the codes 0..16 (vina.py: XS_NAMES)
#define IF_HYD 0xF001u             // C_H F_H Cl_H Br_H I_H
#define IF_DON 0x02A8u             // N_D N_DA O_D O_DA
#define IF_ACC 0x0330u             // N_A N_DA O_A O_DA
#define IF_HAL 0xE000u             // Cl_H Br_H I_H
#define IF_CARBON 0x0003u          // C_H C_P

enum { IF_RING = 0, IF_CATION = 1, IF_ANION = 2, IF_NONE = 3 };

struct IfThr {                     // thresholds as the kernel compares them: lengths in A, angles as cosines
  float hyd, hb, cos_hb, ionic, cp_dist, cp_off, pi_dist, pi_off, cos_face, cos_edge, xb, cos_xd, cos_xmin, cos_xmax, early2;
};

struct IfArgs {
  dbfr_interactions_in in;
  IfThr t;
  dbfr_interactions_out out;
};

// cosine of the angle at p between q and r (NaN when a vector vanishes: every comparison with it is then false)
__device__ __forceinline__ float cos_at(float px, float py, float pz, float qx, float qy, float qz, float rx, float ry, float rz) {
  const float ux = qx - px, uy = qy - py, uz = qz - pz, vx = rx - px, vy = ry - py, vz = rz - pz;
  return (ux * vx + uy * vy + uz * vz) / sqrtf((ux * ux + uy * uy + uz * uz) * (vx * vx + vy * vy + vz * vz));
}

// centre (centroid) and unit normal (Newell's sum in list order) of the first n >= 1 points of p; returns false when the sum vanishes
__device__ __forceinline__ bool centre_normal(const float (&p)[IF_GROUP_W][3], int n, float (&c)[3], float (&nrm)[3]) {
  float s[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < IF_GROUP_W; ++k)
    if (k < n) { s[0] += p[k][0]; s[1] += p[k][1]; s[2] += p[k][2]; }
  c[0] = s[0] / (float)n; c[1] = s[1] / (float)n; c[2] = s[2] / (float)n;
  float a[3] = {0.f, 0.f, 0.f};
  float ux = p[0][0] - c[0], uy = p[0][1] - c[1], uz = p[0][2] - c[2];
  const float fx = ux, fy = uy, fz = uz;
#pragma unroll
  for (int k = 1; k < IF_GROUP_W; ++k)
    if (k < n) {
      const float vx = p[k][0] - c[0], vy = p[k][1] - c[1], vz = p[k][2] - c[2];
      a[0] += uy * vz - uz * vy; a[1] += uz * vx - ux * vz; a[2] += ux * vy - uy * vx;
      ux = vx; uy = vy; uz = vz;
    }
  a[0] += uy * fz - uz * fy; a[1] += uz * fx - ux * fz; a[2] += ux * fy - uy * fx;
  const float len = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  nrm[0] = a[0] / len; nrm[1] = a[1] / len; nrm[2] = a[2] / len;
  return len > 0.f;
}

// distance from the ring centre of the projection onto the ring plane (unit normal n) of the point at v from the centre
__device__ __forceinline__ float plane_offset(float nx, float ny, float nz, float vx, float vy, float vz) {
  const float h = nx * vx + ny * vy + nz * vz;
  return sqrtf(fmaxf((vx * vx + vy * vy + vz * vz) - h * h, 0.f));
}

__global__ __launch_bounds__(IF_THREADS) void k_interactions(IfArgs a) {
  __shared__ float4 lx[IF_MAX_LIG];                         // x, y, z, XS type (as int bits)
  __shared__ int lnb[IF_MAX_LIG][3];                        // bonded heavy neighbours (local, -1 = none)
  __shared__ float4 lgc[IF_MAX_LGRP];                       // group centre, kind (as int bits)
  __shared__ float4 lgn[IF_MAX_LGRP];                       // ring normal
  __shared__ unsigned words[IF_MAX_RES / 2];                // residue r: bits 16 (r & 1) .. of words[r >> 1]
  __shared__ int cnt[IF_KINDS];
  const dbfr_interactions_in& in = a.in;
  __shared__ IfThr o;                                       // the thresholds: read from LDS, not held in scalar registers
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int g = frame_group(in.frame_ptr, in.n_group, f);
  const int k = f - in.frame_ptr[g];
  const int l0 = in.lig_ptr[g], N = in.lig_ptr[g + 1] - l0;
  const int g0 = in.lgrp_ptr[g], LG = in.lgrp_ptr[g + 1] - g0;
  const int m0 = in.pocket_ptr[g], M = in.pocket_ptr[g + 1] - m0;
  const int s0 = in.static_ptr ? in.static_ptr[g] : 0, S = in.static_ptr ? in.static_ptr[g + 1] - s0 : 0;
  const int r0 = in.rgrp_ptr[g], RG = in.rgrp_ptr[g + 1] - r0;
  const int NR = in.res_ptr[g + 1] - in.res_ptr[g];
  const bool res_ok = NR >= 0 && NR <= in.max_res;
  const bool shape_ok = res_ok && N >= 1 && N <= in.max_lig && LG >= 0 && LG <= in.max_lgrp && M >= 0 && S >= 0 && RG >= 0;
  int bad_atom = 0;
  if (tid < IF_KINDS) cnt[tid] = 0;
  if (tid == 0) o = a.t;
  if (res_ok)
    for (int t = tid; t < (NR + 1) / 2; t += IF_THREADS) words[t] = 0u;
  if (shape_ok) {
    const float* lp = in.lig_pos + 3 * (in.lig_pos_off[g] + (long long)k * N);
    for (int i = tid; i < N; i += IF_THREADS) {
      const float x = lp[3 * i], y = lp[3 * i + 1], z = lp[3 * i + 2];
      bad_atom |= !atom_ok(x, y, z);
      const int ty = min(max((int)in.lig_type[l0 + i], 0), 16);
      lx[i] = make_float4(x, y, z, __int_as_float(ty));
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int nb = in.lig_nbr[3 * (size_t)(l0 + i) + j];
        lnb[i][j] = nb < 0 ? -1 : min(nb, N - 1);
      }
    }
  }
  __syncthreads();
  const int MR = M + S;
  const Receptor rec = {in.pocket_pos + 3 * (in.pocket_pos_off[g] + (long long)k * M), in.static_pos + 3 * (size_t)s0, nullptr, nullptr, M};
  if (shape_ok && NR > 0) {
    // ligand groups of this frame
    if (tid < LG) {
      const int* row = in.lgrp + 8 * (size_t)(g0 + tid);
      float p[IF_GROUP_W][3], c[3], nrm[3];
      int n = 0;
#pragma unroll
      for (int j = 0; j < IF_GROUP_W; ++j) {
        const int at = row[1 + j];
        const float4 q = lx[at < 0 ? 0 : min(at, N - 1)];
        p[j][0] = q.x; p[j][1] = q.y; p[j][2] = q.z;
        n += (at >= 0 && n == j);
      }
      int kind = row[0];
      kind = (kind < 0 || kind > IF_ANION || n < 1) ? IF_NONE : kind;
      const bool has_normal = centre_normal(p, max(n, 1), c, nrm);
      if (kind == IF_RING && !(has_normal && n >= 3)) kind = IF_NONE;
      lgc[tid] = make_float4(c[0], c[1], c[2], __int_as_float(kind));
      lgn[tid] = make_float4(nrm[0], nrm[1], nrm[2], 0.f);
    }
    // receptor atoms against the ligand atoms: bits 0, 1, 2, 9
    for (int b = tid; b < MR; b += IF_THREADS) {
      const float* y = rec.pos(b);
      const float yx = y[0], yy = y[1], yz = y[2];
      bad_atom |= !atom_ok(yx, yy, yz);
      const int4 meta = *(const int4*)rec.sel(b, in.pocket_meta + 4 * (size_t)m0, in.static_meta + 4 * (size_t)s0, 4);
      const int tb = min(meta.x & 255, 16);
      const int res = min(max(meta.x >> 8, 0), NR - 1);
      const bool hyd_b = IF_HYD >> tb & 1u, don_b = IF_DON >> tb & 1u, acc_b = IF_ACC >> tb & 1u;
      if (!(hyd_b || don_b || acc_b)) continue;
      float ny[3][3];
      bool nv[3] = {false, false, false}, loaded = false;
      unsigned word = 0u;
      for (int i = 0; i < N; ++i) {
        const float4 q = lx[i];
        const float dx = q.x - yx, dy = q.y - yy, dz = q.z - yz;
        const float d2 = dx * dx + dy * dy + dz * dz;
        if (!(d2 <= o.early2)) continue;
        const float d = sqrtf(d2);
        const int ta = __float_as_int(q.w);
        const bool don_a = IF_DON >> ta & 1u, acc_a = IF_ACC >> ta & 1u;
        if (hyd_b && (IF_HYD >> ta & 1u) && d <= o.hyd) word |= 1u;
        const bool hbd = don_a && acc_b, hba = acc_a && don_b;
        const bool hb = (hbd || hba) && d <= o.hb;
        const bool xb = (IF_HAL >> ta & 1u) && acc_b && d <= o.xb;
        if (!(hb || xb)) continue;
        if (!loaded) {                                      // the receptor atom's bonded neighbours, on the first hit only
          const int nbi[3] = {meta.y, meta.z, meta.w};
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            nv[j] = nbi[j] >= 0;
            const int c = min(max(nbi[j], 0), MR - 1);
            const float* z = rec.pos(c);
            ny[j][0] = z[0]; ny[j][1] = z[1]; ny[j][2] = z[2];
          }
          loaded = true;
        }
        bool hb_ok = true, xb_ok = true;
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (nv[j]) {
            const float c = cos_at(yx, yy, yz, ny[j][0], ny[j][1], ny[j][2], q.x, q.y, q.z);
            hb_ok = hb_ok && c <= o.cos_hb;
            xb_ok = xb_ok && c <= o.cos_xmin && c >= o.cos_xmax;
          }
        bool xd_ok = false;                                 // the halogen's first carbon neighbour
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int nb = lnb[i][j];
          if (nb < 0) continue;
          const float4 x = lx[nb];
          const float c = cos_at(q.x, q.y, q.z, x.x, x.y, x.z, yx, yy, yz);
          hb_ok = hb_ok && c <= o.cos_hb;
          if (xb && (IF_CARBON >> __float_as_int(x.w) & 1u)) {
            xd_ok = c <= o.cos_xd;
            xb_ok = xb_ok && xd_ok;
            break;
          }
        }
        if (hb && hb_ok) word |= (hbd ? 2u : 0u) | (hba ? 4u : 0u);
        if (xb && xb_ok && xd_ok) word |= 512u;
      }
      if (word) atomicOr(&words[res >> 1], word << (16 * (res & 1)));
    }
    __syncthreads();                                        // lgc / lgn complete
    // receptor groups against the ligand groups: bits 3 .. 8
    for (int t = tid; t < RG; t += IF_THREADS) {
      const int4 h0 = *(const int4*)(in.rgrp + 8 * (size_t)(r0 + t)), h1 = *(const int4*)(in.rgrp + 8 * (size_t)(r0 + t) + 4);
      const int at[IF_GROUP_W] = {h0.y, h0.z, h0.w, h1.x, h1.y, h1.z};
      float p[IF_GROUP_W][3], c[3], nrm[3];
      int n = 0;
#pragma unroll
      for (int j = 0; j < IF_GROUP_W; ++j) {
        const int b = min(max(at[j], 0), max(MR - 1, 0));
        const float* y = rec.pos(b);
        const bool use = at[j] >= 0 && MR > 0;
        p[j][0] = use ? y[0] : 0.f; p[j][1] = use ? y[1] : 0.f; p[j][2] = use ? y[2] : 0.f;
        n += (use && n == j);
      }
      int kr = h0.x & 255;
      const int res = min(max(h0.x >> 8, 0), NR - 1);
      kr = (kr > IF_ANION || n < 1) ? IF_NONE : kr;
      const bool has_normal = centre_normal(p, max(n, 1), c, nrm);
      if (kr == IF_RING && !(has_normal && n >= 3)) kr = IF_NONE;
      if (kr == IF_NONE) continue;
      unsigned word = 0u;
      for (int j = 0; j < LG; ++j) {
        const float4 lc = lgc[j], ln = lgn[j];
        const int kl = __float_as_int(lc.w);
        if (kl == IF_NONE) continue;
        const float vx = c[0] - lc.x, vy = c[1] - lc.y, vz = c[2] - lc.z;
        const float d = sqrtf(vx * vx + vy * vy + vz * vz);
        if (kl == IF_CATION && kr == IF_ANION && d <= o.ionic) word |= 8u;
        if (kl == IF_ANION && kr == IF_CATION && d <= o.ionic) word |= 16u;
        if (kl == IF_CATION && kr == IF_RING && d <= o.cp_dist && plane_offset(nrm[0], nrm[1], nrm[2], vx, vy, vz) <= o.cp_off)
          word |= 32u;
        if (kl == IF_RING && kr == IF_CATION && d <= o.cp_dist && plane_offset(ln.x, ln.y, ln.z, vx, vy, vz) <= o.cp_off)
          word |= 64u;
        if (kl == IF_RING && kr == IF_RING && d <= o.pi_dist) {
          const float off = fminf(plane_offset(nrm[0], nrm[1], nrm[2], vx, vy, vz), plane_offset(ln.x, ln.y, ln.z, vx, vy, vz));
          const float cn = fabsf(nrm[0] * ln.x + nrm[1] * ln.y + nrm[2] * ln.z);
          if (off <= o.pi_off) word |= (cn >= o.cos_face ? 128u : 0u) | (cn <= o.cos_edge ? 256u : 0u);
        }
      }
      if (word) atomicOr(&words[res >> 1], word << (16 * (res & 1)));
    }
  }
  const bool bad = __syncthreads_or(bad_atom) || !shape_ok;  // uniform over the workgroup; the LDS words are complete
  // the row, coalesced, and the residues per kind (ballot popcounts: integer sums)
  if (res_ok) {
    int16_t* row = a.out.bits ? a.out.bits + in.bits_off[g] + (long long)k * NR : nullptr;
    int sums[IF_KINDS];
#pragma unroll
    for (int q = 0; q < IF_KINDS; ++q) sums[q] = 0;
    for (int r = tid; r - tid < NR; r += IF_THREADS) {      // every thread runs every trip: the ballots are of whole waves
      const unsigned w = (r < NR && !bad) ? (words[r >> 1] >> (16 * (r & 1))) & 0xffffu : 0u;
      if (r < NR && row) row[r] = (int16_t)w;
#pragma unroll
      for (int q = 0; q < IF_KINDS; ++q) sums[q] += __popcll(__ballot((w >> q) & 1u));
    }
    if (lane == 0)
#pragma unroll
      for (int q = 0; q < IF_KINDS; ++q)
        if (sums[q]) atomicAdd(&cnt[q], sums[q]);
  }
  __syncthreads();
  if (tid < IF_KINDS && a.out.counts) a.out.counts[(size_t)f * IF_KINDS + tid] = bad ? -1 : cnt[tid];
}

// ------------------------------------------------------------------------------------------------ host
static float cos_deg(float deg) { return (float)std::cos((double)deg * 3.14159265358979323846 / 180.0); }

extern "C" int dbfr_interactions(const dbfr_interactions_in* in, const dbfr_interactions_opts* opts, const dbfr_interactions_out* out,
                                 void* hip_stream) {
  const char* fn = "dbfr_interactions";
  if (!in || !out) return arg_err(fn, "null argument");
  if (in->n_group < 0 || in->n_frame < 0) return arg_err(fn, "negative n_group / n_frame");
  if (in->max_lig < 0 || in->max_lig > IF_MAX_LIG) return limit_err(fn, "max_lig (ligand atoms)", in->max_lig, 0, IF_MAX_LIG);
  if (in->max_lgrp < 0 || in->max_lgrp > IF_MAX_LGRP) return limit_err(fn, "max_lgrp (ligand rings and charge centres)", in->max_lgrp, 0, IF_MAX_LGRP);
  if (in->max_res < 0 || in->max_res > IF_MAX_RES) return limit_err(fn, "max_res (residues)", in->max_res, 0, IF_MAX_RES);
  dbfr_interactions_opts o = {4.0f, 3.5f, 90.f, 5.5f, 6.0f, 2.0f, 5.5f, 2.0f, 30.f, 60.f, 4.0f, 135.f, 90.f, 150.f};
  if (opts) o = *opts;
  const float lengths[] = {o.hydrophobic_dist, o.hbond_dist, o.ionic_dist, o.cation_pi_dist, o.cation_pi_offset, o.pi_dist, o.pi_offset,
                           o.xbond_dist};
  const float angles[] = {o.hbond_angle, o.face_angle, o.edge_angle, o.xbond_donor_angle, o.xbond_acceptor_min, o.xbond_acceptor_max};
  for (float v : lengths)
    if (!(v >= 0.f && v <= 100.f)) return arg_err(fn, "a length threshold is NaN or outside [0, 100] A");
  for (float v : angles)
    if (!(v >= 0.f && v <= 180.f)) return arg_err(fn, "an angle threshold is NaN or outside [0, 180] degrees");
  if (in->n_frame == 0) return DBFR_OK;
  if (in->n_group == 0) return arg_err(fn, "frames without groups");
  if (!in->frame_ptr || !in->lig_ptr || !in->lig_pos_off || !in->lig_pos || !in->lig_type || !in->lig_nbr || !in->lgrp_ptr || !in->lgrp ||
      !in->pocket_ptr || !in->pocket_pos_off || !in->pocket_pos || !in->pocket_meta || !in->rgrp_ptr || !in->rgrp || !in->res_ptr ||
      !in->bits_off)
    return arg_err(fn, "frame_ptr / lig_ptr / lig_pos_off / lig_pos / lig_type / lig_nbr / lgrp_ptr / lgrp / pocket_ptr / pocket_pos_off / "
                       "pocket_pos / pocket_meta / rgrp_ptr / rgrp / res_ptr / bits_off missing");
  if (in->static_ptr && (!in->static_pos || !in->static_meta)) return arg_err(fn, "static_ptr given without static_pos / static_meta");
  IfArgs a;
  a.in = *in;
  a.out = *out;
  IfThr& t = a.t;
  t.hyd = o.hydrophobic_dist; t.hb = o.hbond_dist; t.cos_hb = cos_deg(o.hbond_angle); t.ionic = o.ionic_dist;
  t.cp_dist = o.cation_pi_dist; t.cp_off = o.cation_pi_offset; t.pi_dist = o.pi_dist; t.pi_off = o.pi_offset;
  t.cos_face = cos_deg(o.face_angle); t.cos_edge = cos_deg(o.edge_angle); t.xb = o.xbond_dist; t.cos_xd = cos_deg(o.xbond_donor_angle);
  t.cos_xmin = cos_deg(o.xbond_acceptor_min); t.cos_xmax = cos_deg(o.xbond_acceptor_max);
  const float widest = std::fmax(o.hydrophobic_dist, std::fmax(o.hbond_dist, o.xbond_dist)) + IF_EARLY;
  t.early2 = widest * widest;
  HIPCHECK(launch_frames(k_interactions, in->n_frame, IF_THREADS, 0, hip_stream, a));
  return DBFR_OK;
}
