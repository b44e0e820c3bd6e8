// Weight packing of the conv kernels (pack.h): host arithmetic only -- no HIP call, no environment variable -- so that the layouts can be
// checked on a CPU (dbfr_test_pack_conv below, tests/test_pack_host.py) and built into a stand-alone program.
#include <cmath>
#include <cstring>
#include <algorithm>
#include <exception>
#include <map>

#include "pack.h"

static int fail(int code, const std::string& s) { dbfr_set_error(s); return code; }

const char* const conv_tensor_suffix[N_CONV_TENSORS] = {".fc.lin.0.weight", ".fc.lin.0.bias", ".fc.lin.3.weight", ".fc.lin.3.bias", ".batch_norm.mean_shift", ".batch_norm.affine_weight", ".batch_norm.affine_bias"};
void conv_tensor_numel(const ConvSpec& sp, int64_t numel[N_CONV_TENSORS]) {
  int nirr = 0, n0e = 0;
  for (auto& ir : sp.out) { nirr += ir.mul; if (ir.l == 0 && ir.p == 1) n0e += ir.mul; }
  const int64_t K = sp.K, n[N_CONV_TENSORS] = {K * K, K, (int64_t)sp.W * K, sp.W, nirr, nirr, n0e};
  memcpy(numel, n, sizeof n);
}

// ---- What pack_conv and pack_conv2 share: lin.3 rows re-ordered for OWNER accumulation (no atomics, reproducible):
//   an output channel (io, w) is a "pair"; its contributions come from every path into io, all u_in.
//   4 pairs with the same (type, mul1) path sequence form a group processed in lock step: tile =
//   4 quads (one per pair = per MFMA lane group) x the same path and u-quad => path type is tile-uniform.
//   A lane keeps the running message element in registers over the group's tiles and stores it once.
struct Row { int orig; float scale; };   // a lin.3 row and the path factor folded into it; orig = -1: the zero row of a padded channel
struct Pair { int io, w; std::vector<const PathDesc*> paths; };   // paths sorted by (type, -mul1); they point into the ConvSpec
struct Group { std::vector<int> pair_idx; int tiles; int xph; };  // four pairs (-1: padding); xph: reads the second x layout (by_in_off only)

// The pairs of a conv and their groups of four.  vector_only leaves the l = 0 outputs out.  by_in_off (k_conv2 layouts): the pairs of a group also
// read the same input slots, and a group reads ONE of the two scalar input blocks (xph says which).
static int build_groups(const ConvSpec& sp, const std::string& name, bool vector_only, bool by_in_off, std::vector<Pair>& pairs, std::vector<Group>& groups) {
  for (int io = 0; io < (int)sp.out.size(); ++io)
    for (int w = 0; w < sp.out[io].mul; ++w) {
      if (vector_only && sp.out[io].l == 0) continue;
      Pair pr{io, w, {}};
      for (auto& p : sp.paths) if (p.io == io) pr.paths.push_back(&p);
      std::stable_sort(pr.paths.begin(), pr.paths.end(),
                       [](const PathDesc* a, const PathDesc* b) { return a->type != b->type ? a->type < b->type : a->mul1 > b->mul1; });
      pairs.push_back(pr);
    }
  auto sig = [&](const Pair& a) {
    std::string k;
    for (auto* p : a.paths) k += std::to_string(p->type) + ":" + std::to_string(p->mul1) + (by_in_off ? ":" + std::to_string(p->in_off) : "") + ",";
    return k;
  };
  std::map<std::string, std::vector<int>> cls;
  std::vector<std::string> order;
  for (int i = 0; i < (int)pairs.size(); ++i) {
    std::string k = sig(pairs[i]);
    if (!cls.count(k)) order.push_back(k);
    cls[k].push_back(i);
  }
  for (auto& k : order) {
    auto& v = cls[k];
    for (size_t i = 0; i < v.size(); i += 4) {
      Group g;
      for (size_t j = i; j < i + 4; ++j) g.pair_idx.push_back(j < v.size() ? v[j] : -1);
      g.tiles = 0;
      bool hi = false, lo = false;
      for (auto* p : pairs[v[i]].paths) {
        if (p->mul1 % 4) return fail(DBFR_ERR_ARG, "input multiplicity not a multiple of 4 in " + name);
        g.tiles += p->mul1 / 4;
        if (p->in_off >= 120) hi = true;
        if (p->in_off < 48) lo = true;
      }
      // the LDS x row holds 120 floats: [0e|1o|1e] for the groups that read the 48x0e inputs, [0o|1o|1e] for those
      // that read the 48x0o inputs (x[120:168]); no output irrep of this model family reads both
      if (by_in_off && hi && lo) return fail(DBFR_ERR_ARG, "channel group reads both scalar input blocks in " + name);
      g.xph = by_in_off && hi ? 1 : 0;
      groups.push_back(g);
    }
  }
  return DBFR_OK;
}

// Where a run's x offsets point and where a padded channel writes:
//   X_GLOBAL (k_conv):            x_off = the slot's offset in the gathered input row; a padded channel writes the trash column D_out
//   X_LDS (k_conv2 / k_conv2h):   x_off = the position inside the 120-float LDS row (the 48x0o block takes the place of the 48x0e one, RunDesc.meta
//                                 bit 20); a padded channel carries column 255 >= D_out and is never stored
enum XRow { X_GLOBAL, X_LDS };

// One RunDesc per path of group G, and behind `rows` the 16 rows of each of its tiles: [4 lane groups = pairs][4 consecutive u_in].
static int emit_group(const ConvSpec& sp, const std::string& name, const std::vector<Pair>& pairs, const Group& G, XRow xrow, std::vector<RunDesc>& runs, std::vector<Row>& rows) {
  const Pair& lead = pairs[G.pair_idx[0]];
  for (size_t pi = 0; pi < lead.paths.size(); ++pi) {
    const PathDesc* lp = lead.paths[pi];
    RunDesc rd;
    const uint32_t flags = (pi == 0 ? 1u : 0u) | (pi + 1 == lead.paths.size() ? 2u : 0u);
    const uint32_t tile0 = (uint32_t)rows.size() / 16, nt = (uint32_t)lp->mul1 / 4, x_step = 4u * (2 * lp->l1 + 1);
    if (tile0 >= (1u << 20) || nt >= (1u << 12)) return fail(DBFR_ERR_ARG, "conv too large for the run descriptor");
    rd.tile0_n = tile0 | (nt << 20);
    rd.meta = (uint32_t)lp->type | (flags << 4) | ((uint32_t)lp->sh_off << 8) | (x_step << 12) | ((uint32_t)G.xph << 20);
    rd.x_off4 = rd.o_off4 = 0;
    for (int g = 0; g < 4; ++g) {
      const int pidx = G.pair_idx[g];
      const PathDesc* p = pidx >= 0 ? pairs[pidx].paths[pi] : lp;
      if (p->type != lp->type || p->sh_off != lp->sh_off || p->mul1 != lp->mul1 || (xrow == X_LDS && p->in_off != lp->in_off))
        return fail(DBFR_ERR_ARG, "channel group with non-uniform paths in " + name);
      const int d_o = 2 * p->lo + 1;
      uint32_t xo = p->in_off, oo = pidx >= 0 ? p->out_off + pairs[pidx].w * d_o : (uint32_t)sp.D_out;
      if (xrow == X_GLOBAL && (xo > 255 || oo > 255)) return fail(DBFR_ERR_ARG, "irreps too wide for the run descriptor");
      if (xrow == X_LDS) {
        if (xo >= 120) xo -= 120;
        if (pidx < 0) oo = 255u;
        if (xo + 4 * (2 * p->l1 + 1) * (p->mul1 / 4) > 120 || (oo != 255u && (int)oo >= sp.D_out))
          return fail(DBFR_ERR_ARG, "irreps do not fit the k_conv2 row layout in " + name);
      }
      rd.x_off4 |= xo << (8 * g);
      rd.o_off4 |= oo << (8 * g);
    }
    runs.push_back(rd);
    for (int u0 = 0; u0 < lp->mul1; u0 += 4)
      for (int g = 0; g < 4; ++g) {
        const int pidx = G.pair_idx[g];
        const PathDesc* p = pidx >= 0 ? pairs[pidx].paths[pi] : lp;
        for (int r = 0; r < 4; ++r)
          rows.push_back(pidx >= 0 ? Row{p->w_off + (u0 + r) * p->mulo + pairs[pidx].w, p->fold} : Row{-1, 0.f});
      }
  }
  return DBFR_OK;
}

// Rows of W (K columns each) in MFMA A-fragment order: [tile][s4][lane][q] = rows[16 tile + (lane&15)] of W, column 16 s4 + 4 (lane>>4) + q.  The
// reduction index is permuted inside every 16-group (MFMA k-step q of lane group g takes k = 16 s4 + 4 g + q) so that the four B operands a lane
// needs for one A fragment are 4 consecutive floats of its edge's activation row: one ds_read_b128 instead of four ds_read_b32
static std::vector<float> fill_fragments(const float* W, int K, const std::vector<Row>& rows) {
  const int KT = K / 16, n_tiles = (int)rows.size() / 16;
  std::vector<float> out((size_t)n_tiles * KT * 64 * 4);
  for (int t = 0; t < n_tiles; ++t)
    for (int s4 = 0; s4 < KT; ++s4)
      for (int lane = 0; lane < 64; ++lane) {
        const Row& r = rows[16 * t + (lane & 15)];
        for (int q = 0; q < 4; ++q)
          out[(((size_t)t * KT + s4) * 64 + lane) * 4 + q] = r.orig >= 0 ? r.scale * W[(size_t)r.orig * K + 16 * s4 + 4 * (lane >> 4) + q] : 0.f;
      }
  return out;
}
static std::vector<float> fill_bias(const float* B, const std::vector<Row>& rows) {
  std::vector<float> out(rows.size());
  for (size_t i = 0; i < rows.size(); ++i) out[i] = rows[i].orig >= 0 ? rows[i].scale * B[rows[i].orig] : 0.f;
  return out;
}
// lin.0 (K x K) keeps its row order
static std::vector<float> fill_fragments_w1(const float* W1, int K) {
  std::vector<Row> rows(K);
  for (int i = 0; i < K; ++i) rows[i] = Row{i, 1.f};
  return fill_fragments(W1, K, rows);
}

// ---- k_conv layout (conv.hip): groups are dealt to the 4 waves of the workgroup by LPT; tiles are laid out wave-major.
int pack_conv(const ConvTensors& t, int kind, const std::string& name, PackedConv* o) {
  ConvSpec sp = make_conv_spec(kind);
  for (auto& p : sp.paths)
    if (p.type < 0) return fail(DBFR_ERR_ARG, "unsupported tensor-product path in " + name);
  const int K = sp.K;
  int64_t numel[N_CONV_TENSORS];
  conv_tensor_numel(sp, numel);
  std::vector<Pair> pairs; std::vector<Group> groups;
  int rc = build_groups(sp, name, false, false, pairs, groups);
  if (rc) return rc;
  // LPT deal to the 4 waves
  std::vector<int> gorder(groups.size());
  for (size_t i = 0; i < gorder.size(); ++i) gorder[i] = (int)i;
  std::stable_sort(gorder.begin(), gorder.end(), [&](int a, int b) { return groups[a].tiles > groups[b].tiles; });
  std::vector<std::vector<int>> wave_groups(4);
  int wave_load[4] = {0, 0, 0, 0};
  for (int gi : gorder) {
    int best = 0;
    for (int v = 1; v < 4; ++v) if (wave_load[v] < wave_load[best]) best = v;
    wave_groups[best].push_back(gi);
    wave_load[best] += groups[gi].tiles;
  }
  // local search on top of LPT: move / swap groups between the heaviest wave and the others while that lowers the
  // maximum (e.g. W=7776: 24 groups of 15 tiles + 6 of 21 => LPT 126/126/117/117, after refinement 123/123/120/120)
  for (int iter = 0; iter < 64; ++iter) {
    int hi = 0;
    for (int v = 1; v < 4; ++v) if (wave_load[v] > wave_load[hi]) hi = v;
    bool improved = false;
    for (int v = 0; v < 4 && !improved; ++v) {
      if (v == hi) continue;
      for (size_t i = 0; i < wave_groups[hi].size() && !improved; ++i) {
        const int gi = wave_groups[hi][i], ti = groups[gi].tiles;
        // move
        if (std::max(wave_load[hi] - ti, wave_load[v] + ti) < wave_load[hi]) {
          wave_groups[v].push_back(gi); wave_groups[hi].erase(wave_groups[hi].begin() + i);
          wave_load[hi] -= ti; wave_load[v] += ti; improved = true; break;
        }
        for (size_t j = 0; j < wave_groups[v].size(); ++j) {   // swap
          const int gj = wave_groups[v][j], tj = groups[gj].tiles;
          if (tj < ti && std::max(wave_load[hi] - ti + tj, wave_load[v] + ti - tj) < wave_load[hi]) {
            std::swap(wave_groups[hi][i], wave_groups[v][j]);
            wave_load[hi] += tj - ti; wave_load[v] += ti - tj; improved = true; break;
          }
        }
      }
    }
    if (!improved) break;
  }
  ConvW& w = o->w;
  memset(&w, 0, sizeof w);
  std::vector<Row> rows;
  for (int v = 0; v < 4; ++v) {
    std::sort(wave_groups[v].begin(), wave_groups[v].end());
    w.wave_tile0[v] = (int)rows.size() / 16;
    w.wave_run0[v] = (int)o->runs.size();
    for (int gi : wave_groups[v])
      if ((rc = emit_group(sp, name, pairs, groups[gi], X_GLOBAL, o->runs, rows))) return rc;
  }
  w.wave_run0[4] = (int)o->runs.size();
  w.wave_tile0[4] = w.n_tiles = (int)rows.size() / 16;
  w.K = K; w.D_in = sp.D_in; w.D_out = sp.D_out; w.W = sp.W;
  o->W1p = fill_fragments_w1(t.p[T_W1], K);
  o->b1.assign(t.p[T_B1], t.p[T_B1] + K);
  o->W2p = fill_fragments(t.p[T_W2], K, rows);
  o->b2p = fill_bias(t.p[T_B2], rows);
  LNDesc& ln = w.ln;
  ln.nblk = (int)sp.out.size();
  int off = 0;
  for (int i = 0; i < ln.nblk; ++i) {
    ln.mul[i] = sp.out[i].mul; ln.dim[i] = sp.out[i].dim(); ln.off[i] = off;
    ln.is0e[i] = sp.out[i].l == 0 && sp.out[i].p == 1;
    off += ln.mul[i] * ln.dim[i];
  }
  o->mean_shift.assign(t.p[T_MEAN_SHIFT], t.p[T_MEAN_SHIFT] + numel[T_MEAN_SHIFT]);
  o->weight.assign(t.p[T_AFFINE_WEIGHT], t.p[T_AFFINE_WEIGHT] + numel[T_AFFINE_WEIGHT]);
  o->bias.assign(t.p[T_AFFINE_BIAS], t.p[T_AFFINE_BIAS] + numel[T_AFFINE_BIAS]);
  return DBFR_OK;
}

// ---- fp16 tiles (conv2h.hip): tiles [tile0, tile0 + nt) of a [tile][K/16][64][4] fp32 fragment array (K = 144) -> the k_conv2h tile format, all with ONE
// power-of-two factor 2^k (returned).  hi = fp16(v 2^k), lo = fp16(v 2^k - hi), both rounded to nearest even: 2 x 11 significand
// bits + the sign of lo = 23 of fp32's 24.  fp16 has five exponent bits, so 2^k puts the largest |v| of these tiles into
// [2^14, 2^15): pieces of every value within 2^-17 of that maximum stay exact to 22 bits (fp16 subnormals reach down to 2^-24 and
// the matrix pipe keeps them -- tools/exp/split_f16.hip part D), smaller ones keep an absolute error of 2^-40 of the maximum.
// Per tile: [2 pieces][4 k-steps of 32][64][8] -- step s = fp32 k-steps 2s and 2s+1 of the same lane -- then [64 lanes][hi 4 | lo 4]
// for the last 16 k (one 16-byte fragment per lane: the A operand of the x32 MFMA that carries both small products of those 16 k,
// its first half the A operand of the x16 MFMA of the large one), then the tile's 16 bias values (fp32) x 2^k = 9280 B.
#define CH_TILE_BYTES_HOST 9280
static uint16_t h16(float v) { const _Float16 h = (_Float16)v; uint16_t u; memcpy(&u, &h, 2); return u; }
// *depth (may be null) receives the largest d over the rows of these tiles with row maximum 2^(15 - d) after scaling (0 for the row that
// sets the factor): a row with d <= F16_ROW_DEPTH_OK keeps 22 significant bits in its two pieces, a deeper one loses one bit per step
// (relative error 2^(d - 40) of the row's own dot product) -- the model routes such a conv to the three-bf16-piece kernel (bf16 has
// fp32's exponent range), see fallback_convs.
// rinv (may be null): per-ROW factors on top of 2^k -- every row of these tiles is multiplied by the power of two 2^d that puts ITS largest
// magnitude into [2^14, 2^15) (as far as its bias allows), rinv[16 t + row] = 2^-d is what the kernel takes off the accumulator row
// (k_conv2h<.., ROWF>; the hidden layers of k_conv2h / k_convz for W1h).  No row is deep any more: *depth reports what is left (bias-bound rows).
static int pack_f16_tiles(const float* frag, const float* bias16, int tile0, int nt, uint16_t* out, int* depth = nullptr, float* rinv = nullptr) {
  constexpr int KT = 9;
  const size_t tile_h = CH_TILE_BYTES_HOST / 2, tail_off = 8192 / 2, bias_off = 9216 / 2;
  float mx = 0.f;
  for (size_t i = (size_t)tile0 * KT * 256; i < (size_t)(tile0 + nt) * KT * 256; ++i) mx = std::max(mx, fabsf(frag[i]));
  int e = 0;
  if (mx > 0.f) (void)frexpf(mx, &e);            // mx = f 2^e, f in [0.5, 1)
  int k = mx > 0.f ? std::max(-120, std::min(120, 15 - e)) : 0;
  // the bias rows carry 2^k too and meet the per-edge factor (at most 2^64, conv2h.hip) in the accumulator, and the accumulator meets
  // the input features in the contraction: keep |bias| 2^k below 2^48 so that all of it stays a finite fp32 number however small the
  // weights of the run are next to its bias (never binding for weights and biases of comparable size; a run it binds for loses
  // relative precision in its pieces, nothing else)
  float bmx = 0.f;
  for (int i = 16 * tile0; i < 16 * (tile0 + nt); ++i) bmx = std::max(bmx, fabsf(bias16[i]));
  if (bmx > 0.f) { int eb = 0; (void)frexpf(bmx, &eb); k = std::min(k, 48 - eb); }
  const float sc = ldexpf(1.f, k);
  std::vector<int> rowd((size_t)nt * 16, 0);        // extra exponent of every row (0 without per-row factors)
  int dmax = 0;
  for (int t = tile0; t < tile0 + nt; ++t)
    for (int row = 0; row < 16; ++row) {
      float rm = 0.f;
      for (int s4 = 0; s4 < KT; ++s4)
        for (int gq = 0; gq < 4; ++gq)
          for (int q = 0; q < 4; ++q) rm = std::max(rm, fabsf(frag[(((size_t)t * KT + s4) * 64 + 16 * gq + row) * 4 + q]));
      if (rm <= 0.f) continue;                     // (all-zero rows: padded channels)
      int er = 0;
      (void)frexpf(rm, &er);
      int d = 15 - (er + k);
      if (rinv) {
        int up = std::max(d, 0);
        const float br = fabsf(bias16[16 * t + row]);
        if (br > 0.f) { int eb = 0; (void)frexpf(br, &eb); up = std::max(0, std::min(up, 48 - eb - k)); }   // (|bias| 2^(k + d) stays below 2^48, as for k)
        up = std::min(up, 100);
        rowd[(size_t)(t - tile0) * 16 + row] = up;
        d -= up;
      }
      dmax = std::max(dmax, d);
    }
  if (depth) *depth = dmax;
  if (rinv)
    for (int i = 0; i < nt * 16; ++i) rinv[(size_t)tile0 * 16 + i] = ldexpf(1.f, -rowd[i]);
  for (int t = tile0; t < tile0 + nt; ++t) {
    float b[16];
    for (int i = 0; i < 16; ++i) b[i] = bias16[16 * t + i] * ldexpf(sc, rowd[(size_t)(t - tile0) * 16 + i]);
    memcpy(&out[t * tile_h + bias_off], b, 64);
    for (int s4 = 0; s4 < KT; ++s4)
      for (int lane = 0; lane < 64; ++lane)
        for (int q = 0; q < 4; ++q) {
          const float v = frag[(((size_t)t * KT + s4) * 64 + lane) * 4 + q] * ldexpf(sc, rowd[(size_t)(t - tile0) * 16 + (lane & 15)]);
          const _Float16 hi = (_Float16)v;
          const uint16_t pc[2] = {h16(v), h16(v - (float)hi)};
          for (int i = 0; i < 2; ++i) {
            if (s4 < 8) out[t * tile_h + ((size_t)(i * 4 + (s4 >> 1)) * 64 + lane) * 8 + 4 * (s4 & 1) + q] = pc[i];
            else out[t * tile_h + tail_off + (size_t)lane * 8 + 4 * i + q] = pc[i];
          }
        }
  }
  return k;
}

// ---- k_conv2 / k_conv2h layout (conv2.hip, conv2h.hip): same channel-owner row order as pack_conv, but ONE tile sequence for all waves.
// vector_only: the rows that feed an l = 0 output irrep are left out (DBFR_GEMM_REDUCE_FIRST serves them through k_convz); only the fp16 pieces
// are uploaded then, and a conv without l = 1 outputs (torsion convs) gets n_tiles = 0.
int pack_conv2(const ConvTensors& t, int kind, const std::string& name, int rowscale, bool vector_only, PackedConv2* o) {
  ConvSpec sp = make_conv_spec(kind);
  const int K = sp.K;
  if (K != 144) return fail(DBFR_ERR_ARG, "k_conv2 layout is for the K=144 convs");
  const int KT = K / 16;
  std::vector<Pair> pairs; std::vector<Group> groups;
  int rc = build_groups(sp, name, vector_only, true, pairs, groups);
  if (rc) return rc;
  std::stable_sort(groups.begin(), groups.end(), [](const Group& a, const Group& b) { return a.xph < b.xph; });
  std::vector<Row> rows;
  std::vector<RunDesc>& runs = o->runs;
  std::vector<int> group_run0;
  for (const Group& G : groups) {
    group_run0.push_back((int)runs.size());
    if ((rc = emit_group(sp, name, pairs, G, X_LDS, runs, rows))) return rc;
  }
  const int n_tiles = (int)rows.size() / 16;
  o->W2q = fill_fragments(t.p[T_W2], K, rows);
  o->b2q = fill_bias(t.p[T_B2], rows);
  ConvW2& w = o->w;
  memset(&w, 0, sizeof w);
  o->vector_only = vector_only;
  w.D_in = sp.D_in; w.D_out = sp.D_out; w.n_tiles = n_tiles; w.n_runs = (int)runs.size();
  // The same fragments cut into TWO fp16 pieces (conv2h.hip), run by run (a run = the tiles of one tensor-product path of one channel group):
  // pack_f16_tiles above.  k travels in RunDesc.meta bits 24..31; the kernel folds 2^-k into the run's harmonics.
  // A conv with a run whose rows lie further apart than two fp16 pieces hold behind ONE factor (depth > F16_ROW_DEPTH_OK) is packed again with
  // per-ROW factors (W2rinv) and served by k_conv2h<.., ROWF>, which takes them off the accumulator rows: four more vector instructions per edge
  // block and tile instead of the six-product kernel (round 4's fall-back).  rowscale = 0 (developer) keeps the old routing, 2 packs
  // every conv this way.
  o->W2h.assign((size_t)n_tiles * (CH_TILE_BYTES_HOST / 2) + 512, 0);
  std::vector<float> w2rinv((size_t)std::max(n_tiles, 1) * 16, 1.f);
  int depth_max = 0, depth_run = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const bool rowf = pass == 1;
    if (rowf && !(rowscale == 2 || (rowscale == 1 && depth_max > F16_ROW_DEPTH_OK))) break;
    if (rowf) depth_run = depth_max;
    depth_max = 0;
    for (RunDesc& rd : runs) {
      const int tile0 = rd.tile0_n & 0xfffff, nt = rd.tile0_n >> 20;
      int depth = 0;
      const int k = pack_f16_tiles(o->W2q.data(), o->b2q.data(), tile0, nt, o->W2h.data(), &depth, rowf ? w2rinv.data() : nullptr);
      depth_max = std::max(depth_max, depth);
      rd.meta = (rd.meta & 0x00ffffffu) | ((uint32_t)(k & 0xff) << 24);
    }
    if (!rowf) depth_run = depth_max;
    else o->W2rinv = w2rinv;
  }
  // the hidden layer W1 (144 x 144) the same way: nine 16-row tiles with ONE factor 2^k1
  const std::vector<float> w1q = fill_fragments_w1(t.p[T_W1], K);
  o->W1h.assign((size_t)KT * (CH_TILE_BYTES_HOST / 2) + 512, 0);
  int depth1 = 0;
  w.k1 = pack_f16_tiles(w1q.data(), t.p[T_B1], 0, KT, o->W1h.data(), &depth1);
  depth_run = std::max(depth_run, depth1);
  if (rowscale == 2 || (rowscale == 1 && depth1 > F16_ROW_DEPTH_OK)) {
    o->W1rinv.assign((size_t)KT * 16, 1.f);
    w.k1 = pack_f16_tiles(w1q.data(), t.p[T_B1], 0, KT, o->W1h.data(), &depth1, o->W1rinv.data());
  }
  w.f16_depth = std::max(depth_max, depth1);
  w.f16_depth_run = depth_run;
  // contiguous group ranges of near-equal tile count for S = 1, 2, 4, 8
  const int n_g = (int)groups.size();
  int total_tiles = 0;
  for (const Group& G : groups) total_tiles += G.tiles;
  for (int si = 0; si < 4; ++si) {
    const int S = 1 << si;
    int gi = 0, acc = 0;
    for (int p = 0; p < S; ++p) {
      w.part_run[si][p] = gi < n_g ? group_run0[gi] : (int)runs.size();
      const long target = (long)total_tiles * (p + 1) / S;
      while (gi < n_g && (acc + groups[gi].tiles / 2 < target || p == S - 1)) { acc += groups[gi].tiles; ++gi; }
    }
    for (int p = S; p <= 8; ++p) w.part_run[si][p] = (int)runs.size();
  }
  return DBFR_OK;
}

// ---- k_convz layout (convz.hip): reduce-first form of the scalar-output paths (layout: common.h ConvZ).  c tiles of 16 (path, u_in) pairs per output irrep,
// scalar-input paths first (48 = 3 full tiles), then the vector-input ones, padded to a tile; W2' = lin.3 row x fold, bias as k = 144,
// every output ROW (irrep, channel) x its own power of two 2^s (largest |value| into [2^14, 2^15)), cut into two fp16 pieces and stored as the
// A fragments of step B: [c tile][k tile][k-step v][w tile][piece][lane (n' = channel, g')][i] = W2'[c = 16 ct + 4 g' + i % 4,
// k = 16 kt + v + 8 (i / 4), channel 16 wt + n'] -- the order in which step A leaves Z in LDS.
// The hidden layer is the one of the k_conv2 packing of the same conv: its k1 here; api.cpp shares the W1h / W1rinv pointers.
int pack_convz(const ConvTensors& t, int kind, const std::string& name, int k1, PackedConvZ* o) {
  ConvSpec sp = make_conv_spec(kind);
  const int K = sp.K;
  ConvZ& z = o->w;
  memset(&z, 0, sizeof z);
  if (K != 144) return fail(DBFR_ERR_ARG, "k_convz is for the K=144 convs");
  const float *W2 = t.p[T_W2], *B2 = t.p[T_B2];
  struct Col { const PathDesc* p; int u; };
  std::vector<std::vector<Col>> cols;      // per scalar output irrep, padded to tiles (p == nullptr: padding)
  std::vector<int> ios;
  for (int io = 0; io < (int)sp.out.size(); ++io) {
    if (sp.out[io].l != 0) continue;
    if (sp.out[io].mul != NS) return fail(DBFR_ERR_ARG, "scalar output irrep with a multiplicity other than 48 in " + name);
    std::vector<Col> c;
    for (int pass = 0; pass < 2; ++pass)
      for (auto& p : sp.paths) {
        if (p.io != io || p.l1 != pass) continue;
        if (p.l1 != p.l2 || p.lo != 0 || p.l1 > 1) return fail(DBFR_ERR_ARG, "unsupported scalar-output path in " + name);
        for (int u = 0; u < p.mul1; ++u) c.push_back({&p, u});
      }
    int n_scalar = 0;
    for (auto& q : c) n_scalar += q.p->l1 == 0;
    if (n_scalar % 16) return fail(DBFR_ERR_ARG, "scalar-input columns do not fill whole tiles in " + name);
    while (c.size() % 16) c.push_back({nullptr, 0});
    cols.push_back(c);
    ios.push_back(io);
  }
  if (ios.size() > 2) return fail(DBFR_ERR_ARG, "more than two scalar output irreps in " + name);
  z.n_io = (int)ios.size();
  int nct_total = 0;
  for (int i = 0; i < z.n_io; ++i) {
    z.nct[i] = (int)cols[i].size() / 16;
    for (auto& q : cols[i]) z.nc_valid[i] += q.p != nullptr;
    z.ct0[i] = nct_total;
    nct_total += z.nct[i];
    int off = 0;
    for (int j = 0; j < ios[i]; ++j) off += sp.out[j].mul * sp.out[j].dim();
    z.out_off[i] = off;
  }
  if (nct_total > CZ_MAXCT) return fail(DBFR_ERR_ARG, "too many c tiles in " + name);
  o->cdesc.assign((size_t)std::max(nct_total, 1) * 16, 0u);
  o->rowinv.assign((size_t)std::max(z.n_io, 1) * NS, 1.f);
  o->W2z.assign((size_t)nct_total * CZ_NKT * 8 * (CZ_TILE_BYTES / 2) + 512, 0);
  for (int i = 0; i < z.n_io; ++i) {
    const auto& c = cols[i];
    for (size_t j = 0; j < c.size(); ++j)
      if (c[j].p) o->cdesc[(size_t)z.ct0[i] * 16 + j] = (uint32_t)(c[j].p->in_off + c[j].u * (2 * c[j].p->l1 + 1)) | ((uint32_t)c[j].p->l1 << 12) |
                                                    ((uint32_t)c[j].p->sh_off << 16) | 0x80000000u;
    auto wval = [&](int cc, int k, int w) -> float {    // W2'[c, k, w]
      if (cc >= (int)c.size() || !c[cc].p || k > K) return 0.f;
      const PathDesc* p = c[cc].p;
      const size_t row = (size_t)p->w_off + (size_t)c[cc].u * p->mulo + w;
      return p->fold * (k < K ? W2[row * K + k] : B2[row]);
    };
    for (int w = 0; w < NS; ++w) {
      float mx = 0.f;
      for (int cc = 0; cc < (int)c.size(); ++cc)
        for (int k = 0; k <= K; ++k) mx = std::max(mx, fabsf(wval(cc, k, w)));
      int s = 0;
      if (mx > 0.f) { int e = 0; (void)frexpf(mx, &e); s = std::max(-100, std::min(100, 15 - e)); }
      o->rowinv[(size_t)i * NS + w] = ldexpf(1.f, -s);
      const float sc = ldexpf(1.f, s);
      const int wt = w >> 4, np = w & 15;
      for (int ct = 0; ct < z.nct[i]; ++ct)
        for (int kt = 0; kt < CZ_NKT; ++kt)
          for (int v = 0; v < 8; ++v)
            for (int gp = 0; gp < 4; ++gp)
              for (int tt = 0; tt < 8; ++tt) {
                const float val = wval(16 * ct + 4 * gp + (tt & 3), 16 * kt + v + 8 * (tt >> 2), w) * sc;   // Z slot (v, g'' = gp, t): k_local = v + 8 (t / 4), c_local = 4 g'' + t % 4 (convz.hip)
                const _Float16 hi = (_Float16)val;
                const size_t tile = ((size_t)(z.ct0[i] + ct) * CZ_NKT + kt) * 8 + v;
                const size_t base_h = tile * (CZ_TILE_BYTES / 2) + (size_t)(wt * 2) * 512 + (size_t)(16 * gp + np) * 8 + tt;
                o->W2z[base_h] = h16(val);
                o->W2z[base_h + 512] = h16(val - (float)hi);
              }
    }
  }
  z.k1 = k1;
  return DBFR_OK;
}

// ---- test hooks (include/dbfr.h)
extern "C" int dbfr_test_pack_f16_tiles(const float* frag, const float* bias, int32_t n_tiles, void* out, int32_t* k_out) {
  if (!frag || !bias || !out || !k_out || n_tiles <= 0) return fail(DBFR_ERR_ARG, "dbfr_test_pack_f16_tiles: bad argument");
  *k_out = pack_f16_tiles(frag, bias, 0, n_tiles, (uint16_t*)out);
  return DBFR_OK;
}

extern "C" int dbfr_test_pack_f16_rows(const float* frag, const float* bias, int32_t n_tiles, void* out, int32_t* k_out, float* rinv_out, int32_t* depth_out) {
  if (!frag || !bias || !out || !k_out || !rinv_out || n_tiles <= 0) return fail(DBFR_ERR_ARG, "dbfr_test_pack_f16_rows: bad argument");
  int depth = 0;
  *k_out = pack_f16_tiles(frag, bias, 0, n_tiles, (uint16_t*)out, &depth, rinv_out);
  if (depth_out) *depth_out = depth;
  return DBFR_OK;
}

extern "C" int dbfr_test_pack_f16_depth(const float* frag, const float* bias, int32_t n_tiles, int32_t* depth_out, int32_t* depth_ok_out) {
  if (!frag || !bias || !depth_out || n_tiles <= 0) return fail(DBFR_ERR_ARG, "dbfr_test_pack_f16_depth: bad argument");
  std::vector<uint16_t> out((size_t)n_tiles * (CH_TILE_BYTES_HOST / 2) + 512, 0);
  int depth = 0;
  (void)pack_f16_tiles(frag, bias, 0, n_tiles, out.data(), &depth);
  *depth_out = depth;
  if (depth_ok_out) *depth_ok_out = F16_ROW_DEPTH_OK;
  return DBFR_OK;
}

struct Fnv1a64 {
  uint64_t h = 14695981039346656037ull;
  void add(const void* p, size_t n) { for (size_t i = 0; i < n; ++i) { h ^= ((const uint8_t*)p)[i]; h *= 1099511628211ull; } }
  template <typename T> void pod(const T& v) { add(&v, sizeof v); }
};
// the non-pointer members, in declaration order
static void digest(Fnv1a64& f, const ConvW& w) {
  f.pod(w.K); f.pod(w.D_in); f.pod(w.D_out); f.pod(w.n_tiles); f.pod(w.W); f.pod(w.wave_tile0); f.pod(w.wave_run0);
  f.pod(w.ln.nblk); f.pod(w.ln.mul); f.pod(w.ln.dim); f.pod(w.ln.off); f.pod(w.ln.is0e);
}
static void digest(Fnv1a64& f, const ConvW2& w) {
  f.pod(w.D_in); f.pod(w.D_out); f.pod(w.n_tiles); f.pod(w.n_runs); f.pod(w.k1); f.pod(w.f16_depth); f.pod(w.f16_depth_run); f.pod(w.part_run);
}
static void digest(Fnv1a64& f, const ConvZ& z) { f.pod(z.n_io); f.pod(z.nct); f.pod(z.ct0); f.pod(z.out_off); f.pod(z.nc_valid); f.pod(z.k1); }

extern "C" int dbfr_test_pack_conv(int32_t kind, const float* const* tensors7, int32_t rowscale, int64_t* numel7, uint64_t* digests, int32_t digests_cap,
                                   char* names, size_t names_cap, int32_t* flags) {
  if (kind < 0 || kind > 5 || rowscale < 0 || rowscale > 2 || !numel7) return fail(DBFR_ERR_ARG, "dbfr_test_pack_conv: bad argument");
  try {
    conv_tensor_numel(make_conv_spec(kind), numel7);
    if (!tensors7) return 0;
    if (!digests) return fail(DBFR_ERR_ARG, "dbfr_test_pack_conv: bad argument");
    ConvTensors t;
    for (int i = 0; i < N_CONV_TENSORS; ++i)
      if (!(t.p[i] = tensors7[i]) && numel7[i]) return fail(DBFR_ERR_ARG, "dbfr_test_pack_conv: bad argument");
    std::vector<uint64_t> out;
    std::string all;
    Fnv1a64 scalars;
    auto put = [&](const std::string& prefix, auto& packed) {
      each_array(packed, [&](const char* n, const auto& h, const auto&) {
        Fnv1a64 f;
        f.add(h.data(), h.size() * sizeof h[0]);
        out.push_back(h.size() * sizeof h[0]); out.push_back(f.h);
        all += (all.empty() ? "" : ";") + prefix + n;
      });
      digest(scalars, packed.w);
    };
    PackedConv pc; PackedConv2 p2, p2v; PackedConvZ pz;
    int rc = pack_conv(t, kind, "conv", &pc);
    if (!rc) put("conv.", pc);
    if (!rc && kind != 4) {
      rc = pack_conv2(t, kind, "conv", rowscale, false, &p2);
      if (!rc) put("conv2.", p2);
      if (!rc && kind <= 3) { rc = pack_conv2(t, kind, "conv", rowscale, true, &p2v); if (!rc) put("conv2v.", p2v); }
      if (!rc) rc = pack_convz(t, kind, "conv", p2.w.k1, &pz);
      if (!rc) put("convz.", pz);
    }
    if (rc) return rc;
    const int n = (int)out.size() / 2;
    out.push_back(scalars.h);
    if ((int)out.size() > digests_cap || (names && all.size() + 1 > names_cap)) return fail(DBFR_ERR_ARG, "dbfr_test_pack_conv: output buffer too small");
    memcpy(digests, out.data(), out.size() * sizeof(uint64_t));
    if (names) memcpy(names, all.c_str(), all.size() + 1);
    if (flags) *flags = (p2.W2rinv.empty() ? 0 : 1) | (p2.W1rinv.empty() ? 0 : 2) | (p2v.W2rinv.empty() ? 0 : 4) | (p2v.W1rinv.empty() ? 0 : 8);
    return n;
  } catch (const std::exception& e) {
    return fail(DBFR_ERR_ARG, std::string("dbfr_test_pack_conv: ") + e.what());
  }
}
