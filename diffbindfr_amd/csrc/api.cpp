// libdbfr host side: model packing, workspace planning, kernel orchestration, C ABI (include/dbfr.h).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <map>

#include "launch.h"   // the kernel files' interface (+ common.h)
#include "pack.h"

// the lanes (one float4 of message columns each) that hold the scalar-output columns k_convz writes: 12 per irrep from out_off / 4
static unsigned long long convz_sc_lanes(const ConvZ& z) {
  unsigned long long m = 0;
  for (int i = 0; i < z.n_io; ++i) m |= 0xfffull << (z.out_off[i] / 4);
  return m;
}
// HBM bytes per edge of the FUSED conv (what the kernels of this library have to move): edge record (48 embedding floats, 9 harmonics,
// 3 indices), two gathered 48-float rows for the radial MLP, the gathered D_in-float input row, the D_out-float message
static inline double fused_bytes(int D_in, int D_out) { return 4.0 * (48 + 9 + 3 + 48 + 48 + D_in + D_out); }

// AF2 residue constant tables (data only; generated from the reference's protein_constants.py by tests/golden/make_residue_tables.py)
#define RT_TABLE static const
#include "residue_tables.inc"
#undef RT_TABLE

static thread_local std::string g_err;
void dbfr_set_error(const std::string& s) { g_err = s; }
static int fail(int code, const std::string& s) { g_err = s; return code; }

static thread_local bool g_launch_err = false;
bool dbfr_launch_check(hipError_t e, const char* what) {
  if (e == hipSuccess) return false;
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  g_launch_err = true;
  return true;
}
// entry points call this behind their launches: a launcher that gave up (dbfr_launch_check) makes the call fail with DBFR_ERR_HIP
int dbfr_take_launch_error() {
  if (!g_launch_err) return DBFR_OK;
  g_launch_err = false;
  return DBFR_ERR_HIP;
}
static int take_launch_error() { return dbfr_take_launch_error(); }
int dbfr_current_cu_count() {
  static std::atomic<int> cache[64];                     // (zero-initialised; host threads driving different devices may fill it concurrently)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int n = cache[dev].load(std::memory_order_relaxed);
  if (!n) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cache[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

// DBFR_GEMM = f32 | split_f16 | reduce_first: which matrix instruction carries the 144 x W GEMM of the K=144 convs (dbfr_model_set_gemm overrides)
// Anything else -- the retired `split` / `split_l1` / 1 / 2 of rounds 2-4 among it -- is an ERROR (-1; dbfr_model_create fails with DBFR_ERR_ARG): until
// round 6 an unknown value fell silently to the fp32 instruction, a quarter of the default's speed.
static int gemm_from_env() {
  const char* e = getenv("DBFR_GEMM");
  if (!e || !*e) return DBFR_GEMM_DEFAULT;
  if (!strcmp(e, "f32") || !strcmp(e, "0")) return DBFR_GEMM_F32;
  if (!strcmp(e, "split_f16") || !strcmp(e, "3")) return DBFR_GEMM_SPLIT_F16;
  if (!strcmp(e, "reduce_first") || !strcmp(e, "4")) return DBFR_GEMM_REDUCE_FIRST;
  return -1;
}

// Every packed layout of one conv, device resident.  A K=144 conv (an interaction-layer conv or a torsion conv) has all of them; the final conv
// (K=96, k144 false) has `w` alone.
struct ModelConv {
  ConvW w = {};        // k_conv / k_conv_layer
  ConvW2 w2 = {};      // k_conv2 / k_conv2h, every row
  ConvW2 w2v = {};     // ... the l = 1 output rows alone (DBFR_GEMM_REDUCE_FIRST: the scalar outputs go through k_convz)
  bool has_w2v = false;   // (false for the torsion convs: all their outputs are scalars)
  ConvZ z = {};        // reduce-first form of the scalar-output paths (convz.hip)
  bool k144 = false;
};

struct dbfr_model {
  dbfr_model_cfg cfg = {};
  std::vector<void*> allocs;
  ModelConv layer[8][4];   // [l][family]: 0 lig, 1 cross_al, 2 atom, 3 cross_la
  ModelConv final_conv, tor, sc;
  int use_conv2 = -1;
  int gemm_split = 0;  // DBFR_GEMM_*; non-zero: the 144 x W GEMM of the K=144 convs runs on the fp16 matrix pipe with two-piece operands (conv2h.hip; reduce_first:
                       // + convz.hip), any batch size
  int* queue = nullptr;   // [2] unit queue of k_conv2 (re-armed by the kernel itself)
  std::string fallback_convs;   // ';'-separated names of the convs whose weights two fp16 pieces cannot hold (dbfr_model_fallback_convs)
  std::string rowscaled_convs;  // 'name:depth;' of the convs packed with per-row factors (dbfr_model_rowscaled_convs)
  uint32_t layer_fallback = 0;  // bit l: interaction layer l goes through the fp32-instruction kernel k_conv2 whatever the mode (a bias 2^48 above its row); bit 31: the torsion heads
  int* edge_log = nullptr; int edge_log_steps = 0, edge_log_graphs = 0;   // dbfr_model_set_edge_log: caller-owned device buffer [steps][6][graphs], or null
  int* tie_log = nullptr; int tie_log_steps = 0, tie_log_graphs = 0; float tie_tol = 0.f;   // dbfr_model_set_tie_log: likewise, candidate pairs within tie_tol of a cutoff
  Mlp2 lig_node_emb = {}, lig_edge_emb = {}, atom_edge_emb = {}, la_edge_emb = {}, center_edge_emb = {}, tor_edge_emb = {}, sc_edge_emb = {};
  Mlp2 tr_final = {}, rot_final = {}, tor_final = {}, sc_final = {};
  const float* atom_emb[5] = {}; int atom_dims[5] = {};
  const float* atom_lin_t = nullptr;
  const float *gs_lig_off = nullptr, *gs_lig_c = nullptr, *gs_atom_off = nullptr, *gs_atom_c = nullptr;
  const float *gs_cross_off = nullptr, *gs_cross_c = nullptr, *gs_center_off = nullptr, *gs_center_c = nullptr;
  int* a14_group = nullptr;
  // profiling of the dominant kernel
  int profile = 0;
  std::vector<hipEvent_t> ev;
  size_t ev_used = 0;
  double* flops_dev = nullptr;
  double fused_bytes_last = 0;   // third counter as of the last dbfr_profile_read (before its reset)
  double executed_last = 0;      // fourth counter (flops the matrix pipe executed in the K=144 conv launches), likewise
  double useful_last = 0;        // fifth: the executed flops that are not padding
  double form_bytes_last = 0;    // sixth: HBM bytes the form that runs has to move (DBFR_GEMM_REDUCE_FIRST: scalar-output message columns once per segment, inputs read by both kernels)
  double conv_ms_acc = 0; int64_t conv_launches_acc = 0;
};

template <typename T>
static T* upload(dbfr_model* m, const std::vector<T>& h, int* rc) {
  void* d = nullptr;
  size_t bytes = std::max<size_t>(h.size() * sizeof(T), 16);
  if (hipMalloc(&d, bytes) != hipSuccess) { *rc = DBFR_ERR_HIP; g_err = "hipMalloc failed (model weights)"; return nullptr; }
  if (!h.empty() && hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
    *rc = DBFR_ERR_HIP; g_err = "hipMemcpy failed (model weights)"; return nullptr;
  }
  m->allocs.push_back(d);
  return (T*)d;
}

typedef std::map<std::string, const dbfr_tensor*> TMap;

static const float* need(const TMap& tm, const std::string& name, int64_t numel, int* rc) {
  auto it = tm.find(name);
  if (it == tm.end()) { *rc = fail(DBFR_ERR_ARG, "missing tensor '" + name + "'"); return nullptr; }
  if (it->second->numel != numel) {
    *rc = fail(DBFR_ERR_ARG, "tensor '" + name + "' has " + std::to_string(it->second->numel) + " elements, expected " +
                                 std::to_string(numel));
    return nullptr;
  }
  return it->second->data;
}

static int pack_mlp(dbfr_model* m, const TMap& tm, const std::string& name, int in, int hid, int out, bool bias, Mlp2* o) {
  int rc = 0;
  const float* w0 = need(tm, name + ".lin.0.weight", (int64_t)hid * in, &rc);
  const float* w1 = need(tm, name + ".lin.3.weight", (int64_t)out * hid, &rc);
  const float *b0 = nullptr, *b1 = nullptr;
  if (bias) { b0 = need(tm, name + ".lin.0.bias", hid, &rc); b1 = need(tm, name + ".lin.3.bias", out, &rc); }
  if (rc) return rc;
  std::vector<float> w0t((size_t)in * hid), w1t((size_t)hid * out);
  for (int h = 0; h < hid; ++h) for (int i = 0; i < in; ++i) w0t[(size_t)i * hid + h] = w0[(size_t)h * in + i];
  for (int q = 0; q < out; ++q) for (int h = 0; h < hid; ++h) w1t[(size_t)h * out + q] = w1[(size_t)q * hid + h];
  o->in = in; o->hid = hid; o->out = out;
  o->w0t = upload(m, w0t, &rc); o->w1t = upload(m, w1t, &rc);
  o->b0 = o->b1 = nullptr;
  if (bias) {
    o->b0 = upload(m, std::vector<float>(b0, b0 + hid), &rc);
    o->b1 = upload(m, std::vector<float>(b1, b1 + out), &rc);
  }
  return rc;
}

extern "C" int dbfr_model_rowscaled_convs(const dbfr_model* m, char* names, size_t names_cap) {
  if (!m) return fail(DBFR_ERR_ARG, "null model");
  int n = 0;
  for (char c : m->rowscaled_convs) n += c == ';';
  if (names && names_cap) {
    const size_t len = std::min(names_cap - 1, m->rowscaled_convs.size());
    memcpy(names, m->rowscaled_convs.data(), len);
    names[len] = 0;
  }
  return n;
}

extern "C" int dbfr_model_fallback_convs(const dbfr_model* m, char* names, size_t names_cap) {
  if (!m) return fail(DBFR_ERR_ARG, "null model");
  int n = 0;
  for (char c : m->fallback_convs) n += c == ';';
  if (names && names_cap) {
    const size_t len = std::min(names_cap - 1, m->fallback_convs.size());
    memcpy(names, m->fallback_convs.data(), len);
    names[len] = 0;
  }
  return n;
}

// the per-graph read-outs are laid out for a graph capacity: a batch with MORE graphs is refused here, before any launch (a smaller one -- the ragged last
// batch of a sharded run -- fills the first G entries of each row)
static int check_logs(const dbfr_model* m, int G) {
  if (m->edge_log && G > m->edge_log_graphs) return fail(DBFR_ERR_ARG, "dbfr_model_set_edge_log: the buffer was sized for " + std::to_string(m->edge_log_graphs) + " graphs, this batch has " + std::to_string(G));
  if (m->tie_log && G > m->tie_log_graphs) return fail(DBFR_ERR_ARG, "dbfr_model_set_tie_log: the buffer was sized for " + std::to_string(m->tie_log_graphs) + " graphs, this batch has " + std::to_string(G));
  return DBFR_OK;
}

extern "C" int dbfr_model_set_tie_log(dbfr_model* m, int32_t* log_dev, int32_t n_steps_cap, int32_t n_graphs_cap, float tol) {
  if (!m || (log_dev && (n_steps_cap <= 0 || n_graphs_cap <= 0 || !(tol > 0.f)))) return fail(DBFR_ERR_ARG, "dbfr_model_set_tie_log: bad argument");
  m->tie_log = log_dev; m->tie_log_steps = log_dev ? n_steps_cap : 0; m->tie_log_graphs = log_dev ? n_graphs_cap : 0; m->tie_tol = log_dev ? tol : 0.f;
  return DBFR_OK;
}

extern "C" int dbfr_model_set_edge_log(dbfr_model* m, int32_t* log_dev, int32_t n_steps_cap, int32_t n_graphs_cap) {
  if (!m || (log_dev && (n_steps_cap <= 0 || n_graphs_cap <= 0))) return fail(DBFR_ERR_ARG, "dbfr_model_set_edge_log: bad argument");
  m->edge_log = log_dev; m->edge_log_steps = log_dev ? n_steps_cap : 0; m->edge_log_graphs = log_dev ? n_graphs_cap : 0;
  return DBFR_OK;
}

extern "C" int dbfr_model_set_gemm(dbfr_model* m, int32_t mode) {
  if (!m || mode < DBFR_GEMM_F32 || mode > DBFR_GEMM_REDUCE_FIRST || mode == 1 || mode == 2) return fail(DBFR_ERR_ARG, "dbfr_model_set_gemm: bad argument (modes 1 and 2, the three-bf16-piece kernels, were retired with ABI 5 / 4)");
  m->gemm_split = mode;
  return DBFR_OK;
}
extern "C" int dbfr_model_get_gemm(const dbfr_model* m) { return m ? m->gemm_split : DBFR_ERR_ARG; }

extern "C" int dbfr_abi_version(void) { return DBFR_ABI_VERSION; }
#ifndef DBFR_BUILD_ID
#define DBFR_BUILD_ID "unknown"
#endif
extern "C" const char* dbfr_build_id(void) { return DBFR_BUILD_ID; }
extern "C" const char* dbfr_last_error(void) { return g_err.c_str(); }

extern "C" int dbfr_wigner3j(int32_t l1, int32_t l2, int32_t l3, double* out) {
  if (!out || l1 < 0 || l2 < 0 || l3 < 0 || l1 > 4 || l2 > 4 || l3 > 4) return fail(DBFR_ERR_ARG, "bad l");
  std::vector<double> v;
  wigner3j_real(l1, l2, l3, v);
  memcpy(out, v.data(), v.size() * sizeof(double));
  return DBFR_OK;
}

extern "C" int dbfr_conv_paths(int32_t kind, int32_t* t10, int32_t max_paths, int32_t* weight_numel) {
  if (kind < 0 || kind > 5) return fail(DBFR_ERR_ARG, "bad conv kind");
  ConvSpec sp = make_conv_spec(kind);
  if (weight_numel) *weight_numel = sp.W;
  int n = (int)sp.paths.size();
  for (int i = 0; i < n && i < max_paths && t10; ++i) {
    const PathDesc& p = sp.paths[i];
    int32_t* r = t10 + 10 * i;
    r[0] = p.i1; r[1] = p.i2; r[2] = p.io; r[3] = p.l1; r[4] = p.l2; r[5] = p.lo; r[6] = p.mul1; r[7] = p.mulo; r[8] = p.w_off;
    memcpy(&r[9], &p.coeff, 4);
  }
  return n;
}

static int model_create_impl(const dbfr_model_cfg* cfg, const dbfr_tensor* tensors, int32_t n_tensors, dbfr_model** out);
// DBFR_F16_DEPTH (developer): row depth above which a conv leaves the fp16 kernel; 1000 = never (measures what the fall-back protects from)
static int f16_depth_ok() { static const int v = getenv("DBFR_F16_DEPTH") ? atoi(getenv("DBFR_F16_DEPTH")) : F16_ROW_DEPTH_OK; return v; }

extern "C" int dbfr_model_create(const dbfr_model_cfg* cfg, const dbfr_tensor* tensors, int32_t n_tensors,
                                 dbfr_model** out) {
  try {   // weight re-tiling allocates on the host: no exception crosses the C ABI
    return model_create_impl(cfg, tensors, n_tensors, out);
  } catch (const std::exception& e) {
    return fail(DBFR_ERR_ARG, std::string("dbfr_model_create: ") + e.what());
  }
}

// ---- conv weights: the packers of pack.cpp work on the host; here the tensors are looked up and what the packers return goes to the device
static int conv_tensors(const TMap& tm, const std::string& name, int kind, ConvTensors* t) {
  int64_t n[N_CONV_TENSORS];
  conv_tensor_numel(make_conv_spec(kind), n);
  int rc = 0;
  for (int i = 0; i < N_CONV_TENSORS; ++i) t->p[i] = need(tm, name + conv_tensor_suffix[i], n[i], &rc);
  return rc;
}
// Runs one packer (pack(P*)) and sends what it returns to the device: every array, then the scalar fields and the device pointers into *o.  The host copy is freed here, before the next packer runs.
template <typename P, typename D, typename F>
static int pack_upload(dbfr_model* m, D* o, F pack) {
  P p;
  int rc = pack(&p);
  if (rc) return rc;
  each_array(p, [&](const char*, const auto& h, auto& dev) { dev = upload(m, h, &rc); });
  *o = p.w;
  return rc;
}

// Every layout of one K=144 conv (an interaction-layer conv or a torsion conv) into its record: k_conv's, k_conv2 / k_conv2h's, the vector-output
// rows alone (vector_rows; not for the torsion convs, whose outputs are all scalars) and k_convz's.  A conv that two fp16 pieces cannot hold sets
// `fallback_bit` of layer_fallback and is named in fallback_convs, one packed with per-row factors in rowscaled_convs.
static int pack_conv144(dbfr_model* m, const TMap& tm, const std::string& name, int kind, ModelConv* c, bool vector_rows, uint32_t fallback_bit) {
  const int rowscale = getenv("DBFR_F16_ROWSCALE") ? atoi(getenv("DBFR_F16_ROWSCALE")) : 1;   // (pack.h; read at every model creation: a test packs one model this way)
  ConvTensors t;
  int rc = conv_tensors(tm, name, kind, &t);
  if (!rc) rc = pack_upload<PackedConv>(m, &c->w, [&](PackedConv* p) { return pack_conv(t, kind, name, p); });
  if (!rc) rc = pack_upload<PackedConv2>(m, &c->w2, [&](PackedConv2* p) { return pack_conv2(t, kind, name, rowscale, false, p); });
  if (rc) return rc;
  c->w2.W1p = c->w.W1p; c->w2.b1 = c->w.b1;
  if (c->w2.f16_depth > f16_depth_ok()) { m->layer_fallback |= fallback_bit; m->fallback_convs += name + ";"; }
  if (c->w2.W2rinv || c->w2.W1rinv) m->rowscaled_convs += name + ":" + std::to_string(c->w2.f16_depth_run) + ";";
  if (vector_rows) rc = pack_upload<PackedConv2>(m, &c->w2v, [&](PackedConv2* p) { return pack_conv2(t, kind, name, rowscale, true, p); });
  if (!rc) rc = pack_upload<PackedConvZ>(m, &c->z, [&](PackedConvZ* p) { return pack_convz(t, kind, name, c->w2.k1, p); });
  if (rc) return rc;
  if (vector_rows) { c->w2v.W1p = c->w.W1p; c->w2v.b1 = c->w.b1; }
  c->z.W1h = c->w2.W1h; c->z.W1rinv = c->w2.W1rinv;     // k_convz's hidden layer is k_conv2h's
  c->has_w2v = vector_rows; c->k144 = true;
  return DBFR_OK;
}

static int model_create_impl(const dbfr_model_cfg* cfg, const dbfr_tensor* tensors, int32_t n_tensors, dbfr_model** out) {
  if (!cfg || !tensors || !out) return fail(DBFR_ERR_ARG, "null argument");
  if (cfg->ns != NS || cfg->nv != NV || cfg->sh_lmax != 2 || cfg->distance_embed_dim != EMB ||
      cfg->sigma_embed_dim != EMB || cfg->num_conv_layers < 1 || cfg->num_conv_layers > 8)
    return fail(DBFR_ERR_ARG, "unsupported model configuration (need ns=48, nv=12, sh_lmax=2, 32-d embeddings)");
  if (cfg->lig_edge_features + 2 * EMB > 80 || cfg->lig_node_features + EMB > 80)
    return fail(DBFR_ERR_ARG, "ligand feature width too large");
  std::string serr;
  int rc = so3_selftest(serr);
  if (rc) return fail(rc, serr);
  TMap tm;
  for (int i = 0; i < n_tensors; ++i) tm[tensors[i].name] = &tensors[i];
  dbfr_model* m = new dbfr_model();
  m->cfg = *cfg;
  // which fused-conv kernel the K=144 convs use: k_conv2 (persistent, one launch per layer, tail split) wins while a layer
  // is only a few rounds of workgroups (predict.py-sized batches), k_conv (conv.hip) at bench-sized batches.
  // DBFR_CONV2 = 0 / 1 forces one of them, default -1 = by batch size
  m->use_conv2 = getenv("DBFR_CONV2") ? atoi(getenv("DBFR_CONV2")) : -1;
  m->gemm_split = gemm_from_env();
  if (m->gemm_split < 0) rc = fail(DBFR_ERR_ARG, std::string("DBFR_GEMM=") + getenv("DBFR_GEMM") + ": unknown or retired value (f32 | split_f16 | reduce_first)");
  const char* fam[4] = {"lig_conv_layers", "cross_al_conv_layers", "atom_conv_layers", "cross_la_conv_layers"};
  for (int l = 0; l < cfg->num_conv_layers && !rc; ++l)
    for (int f = 0; f < 4 && !rc; ++f)
      rc = pack_conv144(m, tm, std::string(fam[f]) + "." + std::to_string(l), std::min(l, 3), &m->layer[l][f], true, 1u << l);
  ConvTensors final_t;
  if (!rc) rc = conv_tensors(tm, "final_conv", 4, &final_t);
  if (!rc) rc = pack_upload<PackedConv>(m, &m->final_conv.w, [&](PackedConv* p) { return pack_conv(final_t, 4, "final_conv", p); });
  if (!rc) rc = pack_conv144(m, tm, "tor_bond_conv", 5, &m->tor, false, 1u << 31);
  if (!rc && !cfg->no_sc_torsion) rc = pack_conv144(m, tm, "sc_tor_bond_conv", 5, &m->sc, false, 1u << 31);
  if (!rc) rc = pack_mlp(m, tm, "lig_node_embedding", cfg->lig_node_features + EMB, NS, NS, true, &m->lig_node_emb);
  if (!rc) rc = pack_mlp(m, tm, "lig_edge_embedding", cfg->lig_edge_features + 2 * EMB, NS, NS, true, &m->lig_edge_emb);
  if (!rc) rc = pack_mlp(m, tm, "atom_edge_embedding", 2 * EMB, NS, NS, true, &m->atom_edge_emb);
  if (!rc) rc = pack_mlp(m, tm, "la_edge_embedding", 2 * EMB, NS, NS, true, &m->la_edge_emb);
  if (!rc) rc = pack_mlp(m, tm, "center_edge_embedding", 2 * EMB, NS, NS, true, &m->center_edge_emb);
  if (!rc) rc = pack_mlp(m, tm, "tor_edge_embedding", EMB, NS, NS, true, &m->tor_edge_emb);
  if (!rc) rc = pack_mlp(m, tm, "tr_final_layer", 1 + EMB, NS, 1, true, &m->tr_final);
  if (!rc) rc = pack_mlp(m, tm, "rot_final_layer", 1 + EMB, NS, 1, true, &m->rot_final);
  if (!rc) rc = pack_mlp(m, tm, "tor_final_layer", 2 * NS, NS, 1, false, &m->tor_final);
  if (!rc && !cfg->no_sc_torsion) {
    rc = pack_mlp(m, tm, "sc_edge_embedding", EMB, NS, NS, true, &m->sc_edge_emb);
    if (!rc) rc = pack_mlp(m, tm, "sc_tor_final_layer", 2 * NS, NS, 1, false, &m->sc_final);
  }
  const int dims[5] = {37, 22, 4, 21, 2};
  for (int i = 0; i < 5 && !rc; ++i) {
    const float* e = need(tm, "atom_node_embedding.atom_emb_list." + std::to_string(i) + ".weight", (int64_t)dims[i] * NS, &rc);
    if (!rc) { m->atom_emb[i] = upload(m, std::vector<float>(e, e + dims[i] * NS), &rc); m->atom_dims[i] = dims[i]; }
  }
  if (!rc) {
    const float* w = need(tm, "atom_node_embedding.scalar_lin.weight", (int64_t)NS * (NS + EMB), &rc);
    if (!rc) {
      std::vector<float> t((size_t)(NS + EMB) * NS);
      for (int o = 0; o < NS; ++o) for (int i = 0; i < NS + EMB; ++i) t[(size_t)i * NS + o] = w[(size_t)o * (NS + EMB) + i];
      m->atom_lin_t = upload(m, t, &rc);
    }
  }
  struct { const char* n; const float** off; const float** c; } gs[4] = {
      {"lig", &m->gs_lig_off, &m->gs_lig_c}, {"atom", &m->gs_atom_off, &m->gs_atom_c},
      {"cross", &m->gs_cross_off, &m->gs_cross_c}, {"center", &m->gs_center_off, &m->gs_center_c}};
  for (int i = 0; i < 4 && !rc; ++i) {
    const float* off = need(tm, std::string(gs[i].n) + "_distance_expansion.offset", EMB, &rc);
    const float* c = need(tm, std::string(gs[i].n) + "_distance_expansion.coeff", 1, &rc);
    if (!rc) { *gs[i].off = upload(m, std::vector<float>(off, off + EMB), &rc); *gs[i].c = upload(m, std::vector<float>(c, c + 1), &rc); }
  }
  if (!rc) m->a14_group = upload(m, std::vector<int>(kAtom14ToGroup, kAtom14ToGroup + 21 * 14), &rc);
  // profiling counters: flops of the reference algorithm | reference-form bytes | fused-form bytes | executed flops | executed flops that are not padding | bytes of the form that runs
  if (!rc) { m->flops_dev = upload(m, std::vector<double>(6, 0.0), &rc); }
  if (!rc) { m->queue = upload(m, std::vector<int>(4, 0), &rc); }
  if (rc) { dbfr_model_destroy(m); return rc; }
  *out = m;
  return DBFR_OK;
}

extern "C" void dbfr_model_destroy(dbfr_model* m) {
  if (!m) return;
  for (void* p : m->allocs) (void)hipFree(p);
  for (auto e : m->ev) (void)hipEventDestroy(e);
  delete m;
}

// ------------------------------------------------------------------------------------------------ workspace
struct WsEntry { std::string name; size_t offset, bytes; };
struct Bump {
  char* base; size_t off; size_t cap;
  std::vector<WsEntry>* log;
  template <typename T> T* take(size_t n, const char* name = nullptr) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? (T*)(base + off) : nullptr;
    if (log && name) log->push_back({name, off, n * sizeof(T)});
    off += n * sizeof(T);
    return p;
  }
};

struct Ws {
  int* err; int64_t* counters;   // counters [N_SETS]: the segment sum of every edge set's chunks (GraphArgs::chunk_segs; written in profiling mode only)
  int *lig_batch, *atm_batch, *n_cab, *tor_batch, *sc_batch; uint8_t* is_cab;
  float* temb;
  float *c_t, *c_tr_sigma, *c_rot_norm, *c_tor_n2, *c_sc_n2;
  float *s_tr, *s_rot, *s_tor, *s_sc;
  float *lig_x[2], *atom_x[2];
  EdgeSet set[N_SETS];
  // centre set
  int *c_tgt, *c_gth, *c_row_start, *c_row_cnt; float *c_dist, *c_sh, *c_emb;
  float* msg[4]; int conv2; float* gp; float *tor_attr, *sc_attr, *tor_feat, *sc_feat;
  float *xmax_l, *xmax_a;   // [G] largest |feature| of every graph's ligand / pocket nodes in the current layer (k_row_absmax; k_convz's y scale)
  int* n_edges6;  // [8] device counters
};

static void edge_set_take(Bump& b, EdgeSet& S, int cap, int n_targets, int G, int n_graphs, int* n_edges, const char* nm) {
  S.cap = cap; S.n_edges = n_edges;
  std::string p(nm);
  S.tgt = b.take<int>(cap, (p + ".tgt").c_str()); S.gth = b.take<int>(cap, (p + ".gth").c_str());
  S.aux = b.take<int>(cap, (p + ".aux").c_str());
  S.dist = b.take<float>(cap, (p + ".dist").c_str()); S.sh = b.take<float>((size_t)cap * SH_LD, (p + ".sh").c_str());
  S.emb = b.take<float>((size_t)cap * NS, (p + ".emb").c_str());
  S.row_start = b.take<int>(n_targets, (p + ".row_start").c_str()); S.row_cnt = b.take<int>(n_targets, (p + ".row_cnt").c_str());
  S.g_cnt = b.take<int>(G, (p + ".g_cnt").c_str()); S.g_base = b.take<int>(G, (p + ".g_base").c_str());
  S.chunk0 = b.take<int>(n_graphs + 1, (p + ".chunk0").c_str()); S.gedge0 = b.take<int>(n_graphs + 1, (p + ".gedge0").c_str());
  // k_convz's chunk table: a chunk ends after 32 edges, at the end of its graph or with the end of its CZ_MAXSEG-th target (graph.hip k_graph_chunks)
  S.chunk_cap = cap > 0 ? cap / 32 + n_targets / CZ_MAXSEG + n_graphs + 8 : 0;
  S.chunk_es = b.take<int>(std::max(S.chunk_cap, 1), (p + ".chunk_es").c_str()); S.chunk_gl = b.take<int>(std::max(S.chunk_cap, 1), (p + ".chunk_gl").c_str());
  S.seg_first = b.take<uint8_t>(std::max(cap, 1), (p + ".seg_first").c_str());
}

static int plan(const dbfr_model* m, const dbfr_batch* B, const dbfr_limits* lim, char* base, size_t cap, Ws* w,
                size_t* need_bytes, std::vector<WsEntry>* log = nullptr) {
  dbfr_limits L = {24, 64};
  if (lim) { if (lim->aa_avg_neighbors > 0) L.aa_avg_neighbors = lim->aa_avg_neighbors; if (lim->cross_avg_neighbors > 0) L.cross_avg_neighbors = lim->cross_avg_neighbors; }
  Bump b{base, 0, cap, log};
  const int G = B->G, NL = B->NL, NA = B->NA;
  w->err = b.take<int>(16, "err"); w->counters = (int64_t*)b.take<int64_t>(8); w->n_edges6 = b.take<int>(8, "n_edges");
  w->lig_batch = b.take<int>(NL); w->atm_batch = b.take<int>(NA); w->is_cab = b.take<uint8_t>(NA, "is_cab");
  w->n_cab = b.take<int>(G); w->tor_batch = b.take<int>(B->NTOR + 1); w->sc_batch = b.take<int>(B->NSC + 1);
  w->temb = b.take<float>((size_t)G * EMB, "temb");
  w->c_t = b.take<float>(G); w->c_tr_sigma = b.take<float>(G); w->c_rot_norm = b.take<float>(G);
  w->c_tor_n2 = b.take<float>(B->NTOR + 1); w->c_sc_n2 = b.take<float>(B->NSC + 1);
  w->s_tr = b.take<float>(3 * G); w->s_rot = b.take<float>(3 * G); w->s_tor = b.take<float>(B->NTOR + 1); w->s_sc = b.take<float>(B->NSC + 1);
  for (int i = 0; i < 2; ++i) { w->lig_x[i] = b.take<float>((size_t)NL * MAXD, i ? "lig_x1" : "lig_x0"); w->atom_x[i] = b.take<float>((size_t)NA * MAXD, i ? "atom_x1" : "atom_x0"); }
  const int lig_cap = m->cfg.lig_max_neighbors;
  const long cap_ll = (long)NL * std::min(lig_cap + 1, std::max(B->max_nl - 1, 1)) + B->EB;
  const long cap_aa = (long)NA * std::min(L.aa_avg_neighbors, std::max(B->max_na - 1, 1));
  const long cap_x = (long)NL * std::min(B->max_na, 2 * B->max_nr + L.cross_avg_neighbors);
  const long cap_t = (long)B->NTOR * lig_cap, cap_s = m->cfg.no_sc_torsion ? 0 : (long)B->NSC * lig_cap;
  const long caps[N_SETS] = {cap_ll, cap_aa, cap_x, cap_x, cap_t, cap_s};
  const int ntg[N_SETS] = {NL, NA, NL, NA, B->NTOR, B->NSC};
  long maxcap = NL;
  for (int k = 0; k < N_SETS; ++k) {
    if (caps[k] > 0x7fffff00L) return fail(DBFR_ERR_ARG, "batch too large for int32 edge indices; split it");
    static const char* names[N_SETS] = {"ll", "aa", "al", "la", "tor", "sc"};
    edge_set_take(b, w->set[k], (int)caps[k], ntg[k] + 1, G * dbfr_edge_chunks(B->max_na, B->max_nl), G, w->n_edges6 ? w->n_edges6 + k : nullptr, names[k]);
    maxcap = std::max(maxcap, caps[k]);
  }
  w->c_tgt = b.take<int>(NL); w->c_gth = b.take<int>(NL); w->c_dist = b.take<float>(NL); w->c_sh = b.take<float>((size_t)NL * SH_LD, "center.sh");
  w->c_emb = b.take<float>((size_t)NL * NS, "center.emb"); w->c_row_start = b.take<int>(G); w->c_row_cnt = b.take<int>(G);
  // Which conv path a call takes (measured on MI355X, tools/latency_run.py):
  //   largest edge set <= 128 k edges (predict.py-sized batches: 1 complex x 4 poses, -bs 16): persistent k_conv2, one launch per layer;
  //   above: k_conv_layer (the four convs of a layer as one k_conv grid) -- faster than k_conv2 from ~40 poses on.
  static const long conv2_edges = getenv("DBFR_CONV2_EDGES") ? atol(getenv("DBFR_CONV2_EDGES")) : 128 * 1024;
  w->conv2 = m->gemm_split || m->use_conv2 > 0 || (m->use_conv2 < 0 && maxcap <= conv2_edges);
  // every conv of a fused launch writes its own message buffer, sized by its own edge set; msg[0] also serves the centre set and the torsion heads
  // (msg[1]: the side-chain head next to the ligand head in one fused launch)
  const long mc[4] = {std::max({caps[SET_LL], (long)NL, cap_t, cap_s}), std::max(caps[SET_AL], cap_s), caps[SET_AA], caps[SET_LA]};
  for (int i = 0; i < 4; ++i) w->msg[i] = b.take<float>((size_t)std::max(mc[i], 1L) * MAXD, i == 0 ? "msg" : nullptr);
  w->gp = b.take<float>((size_t)G * 12, "gp");
  w->xmax_l = b.take<float>(G, "xmax_l"); w->xmax_a = b.take<float>(G, "xmax_a");
  w->tor_attr = b.take<float>((size_t)(B->NTOR + 1) * NS, "tor_attr"); w->sc_attr = b.take<float>((size_t)(B->NSC + 1) * NS);
  w->tor_feat = b.take<float>((size_t)(B->NTOR + 1) * 2 * NS, "tor_feat"); w->sc_feat = b.take<float>((size_t)(B->NSC + 1) * 2 * NS);
  *need_bytes = b.off + 256;
  return DBFR_OK;
}

static int check_batch(const dbfr_model* m, const dbfr_batch* B) {
  if (!m || !B) return fail(DBFR_ERR_ARG, "null argument");
  if (B->G <= 0 || B->NL <= 0 || B->NA <= 0 || B->NR <= 0) return fail(DBFR_ERR_ARG, "empty batch");
  static_assert(MAX_NL == 256 && MAX_NA == 8192, "the two messages below spell the limits of launch.h out");
  if (B->max_nl > MAX_NL) return fail(DBFR_ERR_ARG, "ligand with more than 256 heavy atoms is not supported");
  if (B->max_na > MAX_NA) return fail(DBFR_ERR_ARG, "pocket with more than 8192 heavy atoms is not supported");
  if (B->max_nl <= 0 || B->max_na <= 0 || B->max_nr <= 0) return fail(DBFR_ERR_ARG, "max_nl/max_na/max_nr must be set");
  return DBFR_OK;
}

extern "C" int dbfr_workspace_bytes(const dbfr_model* m, const dbfr_batch* b, const dbfr_limits* lim, size_t* bytes) {
  int rc = check_batch(m, b);
  if (rc) return rc;
  if (!bytes) return fail(DBFR_ERR_ARG, "null argument");
  Ws w; memset(&w, 0, sizeof w);
  return plan(m, b, lim, nullptr, 0, &w, bytes);
}

// ------------------------------------------------------------------------------------------------ score network
// HIP-event pair around one fused-conv launch on its launch stream (profile mode 1)
static void prof_events(dbfr_model* m, hipEvent_t* e0, hipEvent_t* e1) {
  if (m->ev_used + 2 > m->ev.size()) {
    size_t old = m->ev.size();
    m->ev.resize(old + 512);
    for (size_t i = old; i < m->ev.size(); ++i) (void)hipEventCreate(&m->ev[i]);
  }
  *e0 = m->ev[m->ev_used++]; *e1 = m->ev[m->ev_used++];
}

// One conv site: where a conv finds its edges, the two node tables of its radial MLP (rows idx1 / idx2 of tab1 / tab2 next to the edge embedding), its
// input rows (x, gathered by gth) and where its messages go -- and, for what follows the conv, the CSR rows of the reduction over target nodes.  The
// arguments of every kernel that serves the site (k_conv, k_conv2 / k_conv2h, k_convz) are derived from this one description.
struct ConvSite {
  const int* n_edges; int max_edges; const int *tgt, *gth; const float *emb, *sh;
  const float* tab1; int ld1; const int* idx1;
  const float* tab2; int ld2; const int* idx2;
  const float* x; int ldx;
  float* msg;
  const int *row_start, *row_cnt; const uint8_t* seg_first;                        // the reduction's view (null where the site is not reduced by its builder)
  const int *chunk_es, *chunk_gl, *n_chunks; int max_chunks; const float* xmax;    // k_convz: the chunk table of the edge list, the y scale (or null)
  const int64_t* chunk_segs;                                                       // summed segment counts of that table's chunks (null: a flat list's table has none)
};

static ConvSite flat_site(const int* n_edges, int max_edges, const int* tgt, const int* gth, const float* emb, const float* sh, const float* tab1, int ld1,
                          const int* idx1, const float* tab2, int ld2, const int* idx2, const float* x, int ldx, float* msg) {
  ConvSite s;
  memset(&s, 0, sizeof s);
  s.n_edges = n_edges; s.max_edges = max_edges; s.tgt = tgt; s.gth = gth; s.emb = emb; s.sh = sh;
  s.tab1 = tab1; s.ld1 = ld1; s.idx1 = idx1; s.tab2 = tab2; s.ld2 = ld2; s.idx2 = idx2; s.x = x; s.ldx = ldx; s.msg = msg;
  return s;
}

// ... on an edge set of the workspace; xmax: the per-graph |x| maximum of the node set x belongs to (launch_row_absmax)
static ConvSite conv_site(const EdgeSet& S, int G, const float* tab1, int ld1, const int* idx1, const float* tab2, int ld2, const int* idx2, const float* x,
                          int ldx, float* msg, const float* xmax, const int64_t* chunk_segs) {
  ConvSite s = flat_site(S.n_edges, S.cap, S.tgt, S.gth, S.emb, S.sh, tab1, ld1, idx1, tab2, ld2, idx2, x, ldx, msg);
  s.row_start = S.row_start; s.row_cnt = S.row_cnt; s.seg_first = S.seg_first;
  s.chunk_es = S.chunk_es; s.chunk_gl = S.chunk_gl; s.n_chunks = S.chunk0 + G; s.max_chunks = S.chunk_cap; s.xmax = xmax; s.chunk_segs = chunk_segs;
  return s;
}

static ConvArgs conv_args(const ConvSite& s, const ConvW& cw) {
  ConvArgs a;
  a.n_edges = s.n_edges; a.max_edges = s.max_edges; a.tgt = s.tgt; a.gth = s.gth; a.emb = s.emb; a.sh = s.sh; a.sh_sign = 1.f;
  a.tab1 = s.tab1; a.ld1 = s.ld1; a.idx1 = s.idx1; a.tab2 = s.tab2; a.ld2 = s.ld2; a.idx2 = s.idx2; a.x = s.x; a.ldx = s.ldx;
  a.w = cw; a.msg = s.msg; a.trace = nullptr;
  return a;
}

static Conv2Desc conv2_desc(const ConvSite& s, const ConvW2& cw) {
  Conv2Desc d;
  d.n_edges = s.n_edges; d.max_edges = s.max_edges; d.gth = s.gth; d.emb = s.emb; d.sh = s.sh; d.tab1 = s.tab1; d.ld1 = s.ld1; d.idx1 = s.idx1;
  d.tab2 = s.tab2; d.ld2 = s.ld2; d.idx2 = s.idx2; d.x = s.x; d.ldx = s.ldx; d.w = cw; d.msg = s.msg;
  return d;
}

static ConvZDesc convz_desc(const ConvSite& s, const ConvZ& z, int D_out) {
  ConvZDesc o;
  o.n_edges = s.n_edges; o.max_edges = s.max_edges; o.tgt = s.tgt; o.gth = s.gth; o.emb = s.emb; o.sh = s.sh;
  o.tab1 = s.tab1; o.ld1 = s.ld1; o.idx1 = s.idx1; o.tab2 = s.tab2; o.ld2 = s.ld2; o.idx2 = s.idx2; o.x = s.x; o.ldx = s.ldx;
  o.w = z; o.msg = s.msg; o.D_out = D_out; o.chunk_es = s.chunk_es; o.chunk_gl = s.chunk_gl; o.n_chunks = s.n_chunks; o.max_chunks = s.max_chunks; o.xmax = s.xmax;
  return o;
}

// developer clock read-out of k_conv2h: DBFR_CONV2_TRACE=<file>: the stamps of the LAST traced launch are written at exit.  The device buffer, cleared
// on `st` for the launch that follows, or null
static unsigned long long* conv2_trace(hipStream_t st) {
  static unsigned long long* trace_dev = nullptr;
  static const char* trace_file = getenv("DBFR_CONV2_TRACE");
  if (trace_file && !trace_dev) {
    if (hipMalloc(&trace_dev, 8 * C2_TRACE_CAP * sizeof(unsigned long long)) != hipSuccess) trace_dev = nullptr;
    else atexit([] {
      std::vector<unsigned long long> h(8 * C2_TRACE_CAP);
      if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(h.data(), trace_dev, h.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
        if (FILE* f = fopen(getenv("DBFR_CONV2_TRACE"), "wb")) { fwrite(h.data(), 8, h.size(), f); fclose(f); }
      }
    });
  }
  if (trace_dev) (void)hipMemsetAsync(trace_dev, 0, 8 * C2_TRACE_CAP * sizeof(unsigned long long), st);
  return trace_dev;
}

struct ConvJob { const ModelConv* c; ConvSite site; };

// The one place that maps a group of up to four convs (an interaction layer, the torsion heads present, the final conv, the conv of a test hook) to
// launches, with their profile bookkeeping:
//   per-edge form (!w.conv2, and the K=96 final conv whatever w.conv2 says): a group of four as ONE k_conv_layer grid, any other group one k_conv per job;
//   persistent form, one launch over the group: k_conv2 in DBFR_GEMM_F32 and for a launch that fell back (`fallback`: a conv that even per-row factors
//     cannot fit into two fp16 pieces -- the fp32 instruction), else k_conv2h on every row (DBFR_GEMM_SPLIT_F16);
//   pair form (DBFR_GEMM_REDUCE_FIRST): k_conv2h on the vector-output rows of the convs that have any, then k_convz on the scalar-output rows, both
//     writing the same message buffers.  A site without chunk_segs (the test hook) gets k_convz_useful in front of k_convz.
// profile 1: one HIP-event pair per K=144 launch (the pair form's two launches share one); profile 1 and 2: the counter updates, one k_acc_batch launch
static void conv_group(dbfr_model* m, const Ws& w, const ConvJob* jobs, int n, bool fallback, hipStream_t st) {
  AccBatch ab; ab.count = 0;
  ab.wide = 0;
  auto acc = [&](const int* ne, double coef, double* dst) { if (ab.count < ACC_BATCH_MAX) { ab.n[ab.count] = ne; ab.coef[ab.count] = coef; ab.dst[ab.count] = dst; ++ab.count; } };
  auto acc64 = [&](const int64_t* s, double coef, double* dst) { if (ab.count < ACC_BATCH_MAX) { ab.wide |= 1ull << ab.count; acc(reinterpret_cast<const int*>(s), coef, dst); } };
  // algorithmic flops per edge: radial MLP 2K(K + W) + tensor-product contraction 2*(sum_paths mul1*mulo*dim_o)
  // second counter: HBM bytes the reference's two-kernel form moves per edge (the [E,W] weights once,
  // gathered irreps, harmonics, two int64 indices); the fused kernels never materialise them.  Third: the fused form's bytes
  auto acc_algorithm = [&](const ConvJob& j) {
    const ConvW& cw = j.c->w;
    acc(j.site.n_edges, 2.0 * cw.K * ((double)cw.K + cw.W), m->flops_dev);
    acc(j.site.n_edges, 4.0 * (cw.W + cw.D_in + 9) + 16.0, m->flops_dev + 1);
    acc(j.site.n_edges, fused_bytes(cw.D_in, cw.D_out), m->flops_dev + 2);
  };
  auto timed = [&](bool on, auto&& launch) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (on) {
      prof_events(m, &e0, &e1);
      (void)hipEventRecord(e0, st);
    }
    launch();
    if (on) (void)hipEventRecord(e1, st);
  };
  if (!w.conv2 || !jobs[0].c->k144) {
    // the dominant kernel k_conv<144> only is timed and counted (k_conv<96>: one short launch per step)
    if (n == 4) {   // bench-sized batches in f32 mode: the layer's four convs as ONE k_conv grid
      ConvArgs c4[4];
      for (int i = 0; i < 4; ++i) c4[i] = conv_args(jobs[i].site, jobs[i].c->w);
      timed(m->profile == 1, [&] { launch_conv_layer(c4, st); });
    } else {
      for (int i = 0; i < n; ++i) timed(m->profile == 1 && jobs[i].c->k144, [&] { launch_conv(conv_args(jobs[i].site, jobs[i].c->w), st); });
    }
    for (int i = 0; i < n && m->profile; ++i)
      if (jobs[i].c->k144) acc_algorithm(jobs[i]);
    launch_acc_batch(ab, st);
    return;
  }
  const bool f16 = m->gemm_split >= DBFR_GEMM_SPLIT_F16 && !fallback, pair = f16 && m->gemm_split == DBFR_GEMM_REDUCE_FIRST;
  Conv2Args a;
  memset(&a, 0, sizeof a);
  a.queue = m->queue;
  ConvZArgs za;
  memset(&za, 0, sizeof za);
  za.executed = m->profile ? m->flops_dev + 3 : nullptr;      // k_convz counts the matrix instructions it issues (one atomic per wave and unit)
  bool useful_pass = false;
  int n_tiles[4];   // W2 row tiles the per-edge kernel walks for job i (pair form: the vector-output rows; none for a conv whose outputs are all scalars)
  for (int i = 0; i < n; ++i) {
    const ModelConv& c = *jobs[i].c;
    n_tiles[i] = !pair ? c.w2.n_tiles : c.has_w2v ? c.w2v.n_tiles : 0;
    if (!pair || n_tiles[i] > 0) a.c[a.n_conv++] = conv2_desc(jobs[i].site, pair ? c.w2v : c.w2);
    if (pair) {
      za.c[za.n_conv++] = convz_desc(jobs[i].site, c.z, c.w.D_out);
      useful_pass |= !jobs[i].site.chunk_segs;
    }
  }
  timed(m->profile == 1, [&] {
    a.trace = conv2_trace(st);
    if (pair) {
      if (a.n_conv) launch_conv2h(a, st);
      launch_convz(za, st, useful_pass);
    }
    else if (f16) launch_conv2h(a, st);
    else launch_conv2(a, st);
  });
  for (int i = 0; i < n && m->profile; ++i) {
    const ConvZ& z = jobs[i].c->z;
    const int* ne = jobs[i].site.n_edges;
    acc_algorithm(jobs[i]);
    // what the matrix pipe executes in the per-edge kernel of this launch: `products` MFMA flops per flop of the hidden layer and of the W2 rows it walks
    // (reduce-first: the vector-output rows only; the split kernels of round 2 keep the hidden layer on the fp32 instruction)
    const double rows = 16.0 * n_tiles[i];
    const double ex = f16 ? 3.0 * 2.0 * 144 * (144.0 + rows) : 2.0 * 144 * (144.0 + rows);
    if (!pair || n_tiles[i] > 0) acc(ne, ex, m->flops_dev + 3);
    // ... of which are not padding: everything in the per-edge kernels, except that the pair of DBFR_GEMM_REDUCE_FIRST computes the hidden layer twice
    // (k_convz counts its own instructions and the useful ones among them itself, the hidden layer included)
    if (!pair) acc(ne, ex, m->flops_dev + 4);
    else if (n_tiles[i] > 0) acc(ne, 3.0 * 2.0 * 144 * rows, m->flops_dev + 4);
    // HBM bytes of the form that RUNS: the fused form's, except that the pair reads the edge record and the gathered rows twice and writes the
    // scalar-output message columns once per SEGMENT (k_convz adds 4 x 48 per segment and irrep itself) and one flag byte per edge
    const int D_in = jobs[i].c->w.D_in, D_out = jobs[i].c->w.D_out;
    const double in_bytes = 4.0 * (48 + 9 + 3 + 48 + 48 + D_in);
    if (!pair) acc(ne, fused_bytes(D_in, D_out), m->flops_dev + 5);
    else acc(ne, in_bytes + 1.0 + (n_tiles[i] > 0 ? in_bytes + 4.0 * (D_out - 48 * z.n_io) : 0.0), m->flops_dev + 5);
    // k_convz's own share of the useful flops and of the form bytes, from the edges and the segments of the set's chunks (every edge lies in exactly one chunk:
    // chunk_cap bounds their number, graph.hip k_graph_chunks, so none is cut off and the lengths sum to the edge count): per chunk the hidden layer
    // of its edges; step A the edges x the (path, u) pairs that exist x 145 (the k tile 9: one column); step B one column per segment x (c, k) values x 48;
    // three partial products each; 4 x 48 message bytes per segment and output irrep.  Integers times integer constants: exact in a double.
    if (pair && jobs[i].site.chunk_segs) {
      double ncv = 0.0;
      for (int io = 0; io < z.n_io; ++io) ncv += (double)z.nc_valid[io];
      acc(ne, 6.0 * (144.0 * 144.0 + 145.0 * ncv), m->flops_dev + 4);
      acc64(jobs[i].site.chunk_segs, 6.0 * 145.0 * 48.0 * ncv, m->flops_dev + 4);
      acc64(jobs[i].site.chunk_segs, 4.0 * 48.0 * z.n_io, m->flops_dev + 5);
    }
  }
  launch_acc_batch(ab, st);
}

static int run_score(dbfr_model* m, const dbfr_batch* B, const dbfr_cond* c, const dbfr_scores* out, Ws& w,
                     hipStream_t st, int step = 0) {
  const dbfr_model_cfg& cfg = m->cfg;
  const int G = B->G, NL = B->NL, NA = B->NA;
  launch_time_embed(c->t, G, cfg.emb_scale, w.temb, st);
  // ---- graphs (all six radius-type sets in one count/scan/fill pass)
  GraphArgs ga;
  ga.b = *B; ga.lig_batch = w.lig_batch; ga.atm_batch = w.atm_batch; ga.is_cab = w.is_cab; ga.n_cab = w.n_cab;
  ga.tr_sigma = c->tr_sigma;
  ga.lig_cut2 = cfg.lig_cutoff * cfg.lig_cutoff; ga.atom_cut2 = cfg.atom_cutoff * cfg.atom_cutoff;
  ga.cross_cut2 = cfg.dynamic_max_cross ? 1.0f : cfg.cross_cutoff * cfg.cross_cutoff;
  ga.lig_cap = cfg.lig_max_neighbors; ga.atom_cap = cfg.atom_max_neighbors; ga.dynamic_cross = cfg.dynamic_max_cross;
  for (int k = 0; k < N_SETS; ++k) ga.set[k] = w.set[k];
  ga.err = w.err; ga.step = step; ga.lds_nl = ga.lds_na = 0;
  ga.chunk_segs = m->profile ? reinterpret_cast<long long*>(w.counters) : nullptr;
  dbfr_edge_form(*B, &ga.n_chunk, &ga.lanes);      // one choice of the edge builder's form for every launcher of this call
  launch_edges(ga, false, st);
  // (a launcher that could not prepare its launch left the edge sets unbuilt: nothing below may run on them)
  if (int lrc = take_launch_error()) return lrc;
  if (m->gemm_split == DBFR_GEMM_REDUCE_FIRST) launch_graph_chunks(ga, st);   // per-graph chunks of 32 edges for k_convz
  // (the log rows are laid out for the graph capacity the caller sized the buffer for; a batch with more graphs was refused before anything was launched:
  // check_logs)
  if (m->edge_log && step < m->edge_log_steps) launch_edge_log(ga, m->edge_log + (size_t)step * N_SETS * m->edge_log_graphs, m->edge_log_graphs, st);
  if (m->tie_log && step < m->tie_log_steps) launch_edge_ties(ga, m->tie_log + (size_t)step * N_SETS * m->tie_log_graphs, m->tie_log_graphs, m->tie_tol, st);
  // ---- embeddings
  {
    MlpArgs a; memset(&a, 0, sizeof a);
    a.w = m->lig_node_emb; a.mode = IN_LIGNODE; a.n_rows_max = NL; a.temb = w.temb; a.row_graph_tab = w.lig_batch;
    a.lig_node = B->lig_node; a.nnode = cfg.lig_node_features; a.out = w.lig_x[0];
    launch_mlp(a, st);
  }
  {
    AtomEncArgs a; a.pocket_feat = B->pocket_feat; a.atm_batch = w.atm_batch; a.temb = w.temb;
    for (int i = 0; i < 5; ++i) { a.emb[i] = m->atom_emb[i]; a.dims[i] = m->atom_dims[i]; }
    a.lin_t = m->atom_lin_t; a.NA = NA; a.out = w.atom_x[0];
    launch_atom_encoder(a, st);
  }
  auto edge_mlp = [&](const Mlp2& mw, int mode, const EdgeSet& S, const int* tab, const float* off, const float* co) {
    MlpArgs a; memset(&a, 0, sizeof a);
    a.w = mw; a.mode = mode; a.n_rows_dev = S.n_edges; a.n_rows_max = S.cap; a.temb = w.temb; a.row_graph_tab = tab;
    a.tgt = S.tgt; a.aux = S.aux; a.dist = S.dist; a.bond_feat = B->bond_feat; a.nfeat = cfg.lig_edge_features;
    a.gs_offset = off; a.gs_coeff = co; a.out = S.emb;
    launch_mlp(a, st);
  };
  edge_mlp(m->lig_edge_emb, IN_LIGEDGE, w.set[SET_LL], w.lig_batch, m->gs_lig_off, m->gs_lig_c);
  edge_mlp(m->atom_edge_emb, IN_TG, w.set[SET_AA], w.atm_batch, m->gs_atom_off, m->gs_atom_c);
  edge_mlp(m->la_edge_emb, IN_TG, w.set[SET_AL], w.lig_batch, m->gs_cross_off, m->gs_cross_c);
  edge_mlp(m->la_edge_emb, IN_TG, w.set[SET_LA], w.atm_batch, m->gs_cross_off, m->gs_cross_c);
  // ---- interaction layers
  static const int dims[4] = {48, 84, 120, 168};
  int cur = 0;
  for (int l = 0; l < cfg.num_conv_layers; ++l) {
    const int Di = dims[std::min(l, 3)], Do = dims[std::min(l + 1, 3)];
    const float *lx = w.lig_x[cur], *ax = w.atom_x[cur];
    float *lnew = w.lig_x[cur ^ 1], *anew = w.atom_x[cur ^ 1];
    const EdgeSet &LL = w.set[SET_LL], &AA = w.set[SET_AA], &AL = w.set[SET_AL], &LA = w.set[SET_LA];
    // the four convs of the layer, in family order: the radial MLP reads the target node's row and the source node's, the tensor product the source's;
    // all four read the OLD features
    const ModelConv* mc = m->layer[l];
    const ConvJob jobs[4] = {{&mc[0], conv_site(LL, G, lx, Di, LL.tgt, lx, Di, LL.gth, lx, Di, w.msg[0], w.xmax_l, w.counters + SET_LL)},    // 0 ligand <- ligand
                             {&mc[1], conv_site(AL, G, lx, Di, AL.tgt, ax, Di, AL.gth, ax, Di, w.msg[1], w.xmax_a, w.counters + SET_AL)},    // 1 ligand <- pocket
                             {&mc[2], conv_site(AA, G, ax, Di, AA.tgt, ax, Di, AA.gth, ax, Di, w.msg[2], w.xmax_a, w.counters + SET_AA)},    // 2 pocket <- pocket
                             {&mc[3], conv_site(LA, G, ax, Di, LA.tgt, lx, Di, LA.gth, lx, Di, w.msg[3], w.xmax_l, w.counters + SET_LA)}};   // 3 pocket <- ligand
    const bool fallback = (m->layer_fallback >> l) & 1u;
    const bool rf = m->gemm_split == DBFR_GEMM_REDUCE_FIRST && !fallback;   // the k_convz + k_conv2h pair serves the layer
    // the y scale of k_convz: largest |x| per graph and node set (x = the rows a conv gathers: LL, LA read ligand rows, AL, AA pocket rows)
    if (rf) launch_row_absmax(lx, B->lig_ptr, w.xmax_l, ax, B->atm_ptr, w.xmax_a, Di, Di, G, NA, st);
    conv_group(m, w, jobs, 4, fallback, st);
    ReduceLayerArgs ra;   // one reduction launch: LL then AL into the ligand rows, AA then LA into the pocket rows
    for (int i = 0; i < 4; ++i) {
      const ConvSite& s = jobs[i].site;
      ra.msg[i] = s.msg; ra.row_start[i] = s.row_start; ra.row_cnt[i] = s.row_cnt; ra.ln[i] = mc[i].w.ln;
      ra.first[i] = rf ? s.seg_first : nullptr; ra.sc_lanes[i] = rf ? convz_sc_lanes(mc[i].z) : 0;
    }
    ra.NL = NL; ra.NA = NA; ra.D = Do; ra.D_old = Di; ra.old_l = lx; ra.old_a = ax; ra.out_l = lnew; ra.out_a = anew;
    launch_reduce_ln_layer(ra, st);
    cur ^= 1;
  }
  const int D = dims[std::min(cfg.num_conv_layers, 3)];
  if (D != MAXD) return fail(DBFR_ERR_ARG, "heads need num_conv_layers >= 3");
  const float *lx = w.lig_x[cur], *ax = w.atom_x[cur];
  // ---- translation / rotation head
  launch_center_edges(*B, w.c_tgt, w.c_gth, w.c_dist, w.c_sh, w.c_row_start, w.c_row_cnt, st);
  {
    MlpArgs a; memset(&a, 0, sizeof a);
    a.w = m->center_edge_emb; a.mode = IN_TG; a.n_rows_max = NL; a.temb = w.temb; a.row_graph_tab = w.lig_batch;
    a.dist = w.c_dist; a.gs_offset = m->gs_center_off; a.gs_coeff = m->gs_center_c; a.out = w.c_emb;
    launch_mlp(a, st);
  }
  const ConvJob final_job = {&m->final_conv, flat_site(w.n_edges6 + 7, NL, w.c_tgt, w.c_gth, w.c_emb, w.c_sh, lx, D, w.c_gth, nullptr, 0, w.c_gth, lx, D, w.msg[0])};
  conv_group(m, w, &final_job, 1, false, st);
  launch_reduce_ln(w.msg[0], w.c_row_start, w.c_row_cnt, G, 12, m->final_conv.w.ln, nullptr, 0, w.gp, 12, 2, st);
  {
    TrRotArgs a; a.gp = w.gp; a.temb = w.temb; a.tr_sigma = c->tr_sigma; a.rot_norm = c->rot_score_norm;
    a.tr = m->tr_final; a.rot = m->rot_final; a.G = G; a.scale_by_sigma = cfg.scale_by_sigma; a.tr_out = out->tr;
    a.rot_out = out->rot; a.err = w.err;
    launch_trrot(a, st);
  }
  // ---- the two torsion heads (ligand bonds, side-chain bonds): bond attributes + edge embedding, the conv, reduction + final MLP
  struct TorHead {
    bool on; int n; const EdgeSet* S; ConvJob job;
    const float* nodes; const int *b0, *b1, *bsel; int stride; float* attr;    // launch_bond_attr
    const Mlp2* emb; const float *gs_off, *gs_c;                               // the edge embedding
    const Mlp2* fin; const float* norm2; float *feat, *out;                    // launch_tor_final
  };
  const EdgeSet &T = w.set[SET_TOR], &S = w.set[SET_SC];
  // (a message buffer per head: both convs run before either reduction)
  TorHead heads[2];
  {
    TorHead& h = heads[0];   // ligand torsions: edges bond <- ligand atom
    h.on = B->NTOR > 0; h.n = B->NTOR; h.S = &T;
    h.job = {&m->tor, conv_site(T, G, lx, D, T.gth, w.tor_attr, NS, T.tgt, lx, D, w.msg[0], w.xmax_l, w.counters + SET_TOR)};
    h.nodes = lx; h.b0 = B->bond_src; h.b1 = B->bond_dst; h.bsel = B->tor_bond; h.stride = 0; h.attr = w.tor_attr;
    h.emb = &m->tor_edge_emb; h.gs_off = m->gs_lig_off; h.gs_c = m->gs_lig_c;
    h.fin = &m->tor_final; h.norm2 = c->tor_score_norm2; h.feat = w.tor_feat; h.out = out->tor;
  }
  {
    TorHead& h = heads[1];   // side-chain torsions: edges bond <- pocket atom
    h.on = !cfg.no_sc_torsion && B->NSC > 0; h.n = B->NSC; h.S = &S;
    h.job = {&m->sc, conv_site(S, G, ax, D, S.gth, w.sc_attr, NS, S.tgt, ax, D, w.msg[1], w.xmax_a, w.counters + SET_SC)};
    h.nodes = ax; h.b0 = B->sc_bond; h.b1 = nullptr; h.bsel = nullptr; h.stride = 2; h.attr = w.sc_attr;
    h.emb = &m->sc_edge_emb; h.gs_off = m->gs_atom_off; h.gs_c = m->gs_atom_c;
    h.fin = &m->sc_final; h.norm2 = c->sc_tor_score_norm2; h.feat = w.sc_feat; h.out = out->sc_tor;
  }
  const bool fallback = (m->layer_fallback >> 31) & 1u;
  const bool rf = m->gemm_split == DBFR_GEMM_REDUCE_FIRST && !fallback;
  auto prologue = [&](const TorHead& h) {
    launch_bond_attr(h.nodes, D, h.b0, h.b1, h.bsel, h.stride, h.n, h.attr, st);
    MlpArgs a; memset(&a, 0, sizeof a);
    a.w = *h.emb; a.mode = IN_G; a.n_rows_dev = h.S->n_edges; a.n_rows_max = h.S->cap; a.dist = h.S->dist;
    a.gs_offset = h.gs_off; a.gs_coeff = h.gs_c; a.out = h.S->emb;
    launch_mlp(a, st);
  };
  auto epilogue = [&](const TorHead& h) {
    const ConvSite& s = h.job.site;
    if (rf) launch_reduce_ln(s.msg, s.row_start, s.row_cnt, h.n, 2 * NS, h.job.c->w.ln, nullptr, 0, h.feat, 2 * NS, 2, st, s.seg_first, convz_sc_lanes(h.job.c->z));
    else launch_reduce_ln(s.msg, s.row_start, s.row_cnt, h.n, 2 * NS, h.job.c->w.ln, nullptr, 0, h.feat, 2 * NS, 2, st);
    launch_tor_final(h.feat, *h.fin, h.norm2, cfg.scale_by_sigma, h.n, h.out, st);
  };
  // both prologues, the convs of the heads present as ONE group, both epilogues
  if (rf) launch_row_absmax(lx, B->lig_ptr, w.xmax_l, ax, B->atm_ptr, w.xmax_a, D, D, G, NA, st);
  ConvJob jobs[2]; int nj = 0;
  for (const TorHead& h : heads) {
    if (!h.on) continue;
    prologue(h);
    jobs[nj++] = h.job;
  }
  if (nj) conv_group(m, w, jobs, nj, fallback, st);
  for (const TorHead& h : heads)
    if (h.on) epilogue(h);
  return DBFR_OK;
}

static int begin(dbfr_model* m, const dbfr_batch* B, void* workspace, size_t wbytes, const dbfr_limits* lim, Ws* w,
                 hipStream_t st) {
  g_launch_err = false;                                  // (a flag an earlier, failed call left on this thread is not this call's)
  int rc = check_batch(m, B);
  if (rc) return rc;
  rc = check_logs(m, B->G);
  if (rc) return rc;
  if (!workspace) return fail(DBFR_ERR_ARG, "null workspace");
  size_t needb = 0;
  memset(w, 0, sizeof *w);
  rc = plan(m, B, lim, (char*)workspace, wbytes, w, &needb);
  if (rc) return rc;
  if (needb > wbytes) return fail(DBFR_ERR_ARG, "workspace too small: need " + std::to_string(needb) + " bytes");
  HIPCHECK(hipMemsetAsync(workspace, 0, 1024, st));   // err @0, counters @256, n_edges6 @512
  if (w->conv2) HIPCHECK(hipMemsetAsync(m->queue, 0, 16, st));   // the kernel re-arms it itself; this covers an aborted run
  launch_set_int(w->n_edges6 + 7, B->NL, st);           // the centre set has exactly one edge per ligand atom
  launch_batch_vectors(*B, w->lig_batch, w->atm_batch, w->is_cab, w->n_cab, w->tor_batch, w->sc_batch, st);
  return DBFR_OK;
}

extern "C" int dbfr_score(dbfr_model* m, const dbfr_batch* b, const dbfr_cond* cond, const dbfr_scores* out,
                          void* workspace, size_t workspace_bytes, const dbfr_limits* lim, void* hip_stream) {
  if (!cond || !out) return fail(DBFR_ERR_ARG, "null argument");
  hipStream_t st = (hipStream_t)hip_stream;
  Ws w;
  int rc = begin(m, b, workspace, workspace_bytes, lim, &w, st);
  if (rc) return rc;
  rc = run_score(m, b, cond, out, w, st);
  if (rc) return rc;
  HIPCHECK(hipGetLastError());
  return take_launch_error();
}

// The update half of one denoise step (scFlex.py:154-230): scores + this step's noise slices -> new ligand coordinates, chi angles and
// side chains.  dbfr_sample_range and the test hook dbfr_test_sde_step both go through here.
static void pose_update(const dbfr_model* m, const dbfr_batch* b, const dbfr_step& sp, const dbfr_scores& sc, const float* z_tr,
                        const float* z_rot, const float* z_tor, const float* z_sc, float* traj_lig, float* atom14_out,
                        float* traj_atom14, int* err, hipStream_t st) {
  SdeLigArgs la;
  la.b = *b; la.tr_score = sc.tr; la.rot_score = sc.rot; la.tor_score = sc.tor;
  la.z_tr = z_tr; la.z_rot = z_rot; la.z_tor = z_tor;
  la.dt = sp.dt; la.tr_g2 = sp.tr_g2; la.tr_gsdt = sp.tr_gsdt; la.rot_g2 = sp.rot_g2; la.rot_gsdt = sp.rot_gsdt;
  la.tor_g2 = sp.tor_g2; la.tor_gsdt = sp.tor_gsdt;
  la.traj = traj_lig;
  la.err = err;
  launch_sde_ligand(la, st);
  if (!m->cfg.no_sc_torsion)
    launch_sidechain(*b, sc.sc_tor, z_sc, sp.dt, sp.sc_g2, sp.sc_gsdt, m->a14_group, atom14_out, traj_atom14, err, st);
}

extern "C" int dbfr_sample_range(dbfr_model* m, const dbfr_batch* b, const dbfr_step* steps, int32_t n_steps,
                                 int32_t step_begin, const dbfr_noise* noise, float* atom14_out, float* traj_lig,
                                 float* traj_atom14, void* workspace, size_t workspace_bytes, const dbfr_limits* lim,
                                 void* hip_stream) {
  if (!steps || n_steps <= 0 || !noise) return fail(DBFR_ERR_ARG, "null argument");
  if (step_begin < 0 || step_begin >= n_steps) return fail(DBFR_ERR_ARG, "step_begin out of range");
  hipStream_t st = (hipStream_t)hip_stream;
  Ws w;
  int rc = begin(m, b, workspace, workspace_bytes, lim, &w, st);
  if (rc) return rc;
  const int G = b->G;
  for (int s = step_begin; s < n_steps; ++s) {
    const dbfr_step& sp = steps[s];
    // set_time (scFlex.py:104-122): uniform conditioning over the batch
    launch_fill(w.c_t, sp.t, G, st);
    launch_fill(w.c_tr_sigma, sp.tr_sigma, G, st);
    launch_fill(w.c_rot_norm, sp.rot_score_norm, G, st);
    launch_fill(w.c_tor_n2, sp.tor_score_norm2, b->NTOR, st);
    launch_fill(w.c_sc_n2, sp.tor_score_norm2, b->NSC, st);
    dbfr_cond c = {w.c_t, w.c_tr_sigma, w.c_rot_norm, w.c_tor_n2, w.c_sc_n2};
    dbfr_scores sc = {w.s_tr, w.s_rot, w.s_tor, w.s_sc};
    rc = run_score(m, b, &c, &sc, w, st, s);
    if (rc) return rc;
    pose_update(m, b, sp, sc, noise->z_tr + (size_t)s * G * 3, noise->z_rot + (size_t)s * G * 3, noise->z_tor + (size_t)s * b->NTOR,
                noise->z_sc + (size_t)s * b->NSC, traj_lig ? traj_lig + (size_t)s * b->NL * 3 : nullptr,
                s == n_steps - 1 ? atom14_out : nullptr, traj_atom14 ? traj_atom14 + (size_t)s * b->NR * 42 : nullptr, w.err, st);
  }
  HIPCHECK(hipGetLastError());
  return take_launch_error();
}

extern "C" int dbfr_sample(dbfr_model* m, const dbfr_batch* b, const dbfr_step* steps, int32_t n_steps,
                           const dbfr_noise* noise, float* atom14_out, float* traj_lig, float* traj_atom14,
                           void* workspace, size_t workspace_bytes, const dbfr_limits* lim, void* hip_stream) {
  return dbfr_sample_range(m, b, steps, n_steps, 0, noise, atom14_out, traj_lig, traj_atom14, workspace, workspace_bytes, lim,
                           hip_stream);
}

extern "C" int dbfr_capacity_report(void* workspace, void* hip_stream, int32_t* first_failed_step, int64_t* needed_edges) {
  if (!workspace) return fail(DBFR_ERR_ARG, "null workspace");
  HIPCHECK(hipStreamSynchronize((hipStream_t)hip_stream));
  int h[16];
  HIPCHECK(hipMemcpy(h, workspace, sizeof h, hipMemcpyDeviceToHost));   // err block @0 (plan())
  if (first_failed_step) *first_failed_step = h[1] - 1;
  if (needed_edges) {   // dbfr_status_sync's counter order: lig, atom, cross(al), -, tor, sc_tor, cross(la), -
    needed_edges[0] = h[8 + SET_LL]; needed_edges[1] = h[8 + SET_AA]; needed_edges[2] = h[8 + SET_AL]; needed_edges[3] = 0;
    needed_edges[4] = h[8 + SET_TOR]; needed_edges[5] = h[8 + SET_SC]; needed_edges[6] = h[8 + SET_LA]; needed_edges[7] = 0;
  }
  return DBFR_OK;
}

extern "C" int dbfr_status_sync(void* workspace, void* hip_stream, int64_t* counters) {
  if (!workspace) return fail(DBFR_ERR_ARG, "null workspace");
  hipStream_t st = (hipStream_t)hip_stream;
  HIPCHECK(hipStreamSynchronize(st));
  int h[16 + 16 + 8];
  HIPCHECK(hipMemcpy(h, workspace, sizeof h, hipMemcpyDeviceToHost));
  // layout of plan(): err[16] @0 (64 B), counters[8] @256, n_edges6[8] @512
  int err = h[0];
  if (counters) {
    int ne[8];
    HIPCHECK(hipMemcpy(ne, (char*)workspace + 512, sizeof ne, hipMemcpyDeviceToHost));
    counters[0] = ne[SET_LL]; counters[1] = ne[SET_AA]; counters[2] = ne[SET_AL]; counters[3] = ne[7];
    counters[4] = ne[SET_TOR]; counters[5] = ne[SET_SC]; counters[6] = ne[SET_LA]; counters[7] = 0;
  }
  // device status word is a bit mask: 1 = an edge list overflowed its capacity, 2 = numeric check failed
  if (err & 1) return fail(DBFR_ERR_CAPACITY, "edge capacity exceeded: raise dbfr_limits");
  if (err & 2) return fail(DBFR_ERR_NUMERIC, "non-finite score or Kabsch determinant check failed");
  return DBFR_OK;
}

extern "C" int dbfr_init_poses(const dbfr_model* m, const dbfr_batch* b, const dbfr_init_tape* tape, float* atom14_out,
                               void* hip_stream) {
  int rc = check_batch(m, b);
  if (rc) return rc;
  if (!tape || !tape->rot || !tape->tr || !tape->sc_u || (b->NTOR > 0 && !tape->tor_u))
    return fail(DBFR_ERR_ARG, "null init tape");
  launch_init_poses(*b, *tape, m->a14_group, atom14_out, (hipStream_t)hip_stream);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

extern "C" int dbfr_extract_templates(int32_t n_res, const int32_t* aatype, const float* atom14_pos, float* backbone_transl,
                                      float* backbone_rots, float* default_frame, float* rigid_group_positions,
                                      float* torsion_angle, void* hip_stream) {
  if (n_res < 0 || !aatype || !atom14_pos || !backbone_transl || !backbone_rots || !default_frame || !rigid_group_positions ||
      !torsion_angle)
    return fail(DBFR_ERR_ARG, "null argument");
  launch_extract_templates(n_res, aatype, atom14_pos, backbone_transl, backbone_rots, default_frame, rigid_group_positions,
                           torsion_angle, (hipStream_t)hip_stream);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

extern "C" int dbfr_select_pocket(int32_t n_prot, int32_t n_res_total, const int32_t* res_ptr, int32_t atoms_per_res, const float* atom_pos,
                                  const float* atom_mask, const int32_t* ref_ptr, const float* ref_pos, double cutoff,
                                  int32_t max_neighbors, float* min_dist2, uint8_t* res_mask, void* hip_stream) {
  if (n_prot < 0 || n_res_total < 0 || atoms_per_res < 1) return fail(DBFR_ERR_ARG, "bad size");
  if (n_prot == 0 || n_res_total == 0) return DBFR_OK;
  if (!res_ptr || !atom_pos || !atom_mask || !ref_ptr || !ref_pos || !min_dist2 || !res_mask) return fail(DBFR_ERR_ARG, "null argument");
  // the reference compares float32 distances with the Python double cutoff ** 2 cast to float32
  launch_select_pocket(n_prot, n_res_total, res_ptr, atoms_per_res, atom_pos, atom_mask, ref_ptr, ref_pos, (float)(cutoff * cutoff),
                       max_neighbors, min_dist2, res_mask, (hipStream_t)hip_stream);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

extern "C" int dbfr_profile_enable(dbfr_model* m, int32_t on) {
  if (!m) return fail(DBFR_ERR_ARG, "null model");
  m->profile = on;
  return DBFR_OK;
}

extern "C" int dbfr_profile_read(dbfr_model* m, double* conv_ms, int64_t* conv_launches, double* conv_flops,
                                 double* ref_form_bytes, int32_t reset) {
  if (!m) return fail(DBFR_ERR_ARG, "null model");
  HIPCHECK(hipDeviceSynchronize());
  for (size_t i = 0; i + 1 < m->ev_used; i += 2) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, m->ev[i], m->ev[i + 1]) == hipSuccess) { m->conv_ms_acc += ms; m->conv_launches_acc++; }
  }
  m->ev_used = 0;
  double fl[6] = {0, 0, 0, 0, 0, 0};
  HIPCHECK(hipMemcpy(fl, m->flops_dev, sizeof fl, hipMemcpyDeviceToHost));
  m->fused_bytes_last = fl[2];
  m->executed_last = fl[3];
  m->useful_last = fl[4];
  m->form_bytes_last = fl[5];
  if (conv_ms) *conv_ms = m->conv_ms_acc;
  if (conv_launches) *conv_launches = m->conv_launches_acc;
  if (conv_flops) *conv_flops = fl[0];
  if (ref_form_bytes) *ref_form_bytes = fl[1];
  if (reset) { m->conv_ms_acc = 0; m->conv_launches_acc = 0; HIPCHECK(hipMemset(m->flops_dev, 0, 6 * sizeof(double))); }
  return DBFR_OK;
}

extern "C" int dbfr_profile_executed_flops(const dbfr_model* m, double* executed_flops) {
  if (!m || !executed_flops) return fail(DBFR_ERR_ARG, "null argument");
  *executed_flops = m->executed_last;
  return DBFR_OK;
}

extern "C" int dbfr_profile_useful_flops(const dbfr_model* m, double* useful_flops, double* form_bytes) {
  if (!m || (!useful_flops && !form_bytes)) return fail(DBFR_ERR_ARG, "null argument");
  if (useful_flops) *useful_flops = m->useful_last;
  if (form_bytes) *form_bytes = m->form_bytes_last;
  return DBFR_OK;
}

extern "C" int dbfr_profile_fused_bytes(const dbfr_model* m, double* fused_form_bytes) {
  if (!m || !fused_form_bytes) return fail(DBFR_ERR_ARG, "null argument");
  *fused_form_bytes = m->fused_bytes_last;
  return DBFR_OK;
}

// test hook: named offsets of the internal buffers inside the workspace
extern "C" int dbfr_workspace_layout(const dbfr_model* m, const dbfr_batch* b, const dbfr_limits* lim, char* names,
                                     size_t names_cap, size_t* offsets, size_t* bytes, int32_t max_entries) {
  int rc = check_batch(m, b);
  if (rc) return rc;
  std::vector<WsEntry> log;
  Ws w; memset(&w, 0, sizeof w);
  size_t nb = 0;
  rc = plan(m, b, lim, nullptr, 0, &w, &nb, &log);
  if (rc) return rc;
  size_t pos = 0;
  int n = 0;
  for (auto& e : log) {
    if (n >= max_entries || pos + e.name.size() + 2 > names_cap) break;
    memcpy(names + pos, e.name.c_str(), e.name.size());
    pos += e.name.size();
    names[pos++] = ';';
    offsets[n] = e.offset; bytes[n] = e.bytes;
    ++n;
  }
  names[pos] = 0;
  return n;
}

// ------------------------------------------------------------------------------------------------ unit-test hooks
// the record of a conv by the hooks' (layer, family) address: an interaction-layer conv, -1 the final conv, -2 / -3 the torsion convs; or null
static const ModelConv* pick_conv(const dbfr_model* m, int layer, int family) {
  if (layer >= 0 && layer < m->cfg.num_conv_layers && family >= 0 && family < 4) return &m->layer[layer][family];
  if (layer == -1) return &m->final_conv;
  if (layer == -2) return &m->tor;
  if (layer == -3 && !m->cfg.no_sc_torsion) return &m->sc;
  return nullptr;
}

static int test_conv_impl(dbfr_model* m, bool conv2, int32_t layer, int32_t family, int32_t n_edges, const int32_t* n_edges_dev,
                          const int32_t* tgt, const int32_t* gth, const float* emb, const float* sh, const float* tab1, int32_t ld1,
                          const int32_t* idx1, const float* tab2, int32_t ld2, const int32_t* idx2, const float* x, int32_t ldx,
                          float* msg, void* hip_stream) {
  if (!m) return fail(DBFR_ERR_ARG, "null model");
  g_launch_err = false;
  const ModelConv* c = pick_conv(m, layer, family);
  if (!c) return fail(DBFR_ERR_ARG, "no such conv");
  hipStream_t st = (hipStream_t)hip_stream;
  ConvJob job = {c, flat_site(n_edges_dev, n_edges, tgt, gth, emb, sh, tab1, ld1, idx1, tab2, ld2, idx2, x, ldx, msg)};
  bool deep = false;
  if (conv2) {
    if (!c->k144) return fail(DBFR_ERR_ARG, "k_conv2 serves the K=144 convs");
    deep = c->w2.f16_depth > f16_depth_ok();   // (the hook decides per conv; a fused launch of run_score by its layer's bit of layer_fallback)
    const bool rf = m->gemm_split == DBFR_GEMM_REDUCE_FIRST && !deep;   // (the message buffer then holds segment sums in the segments' first rows: include/dbfr.h)
    // k_convz's chunk table for this flat edge list, in a scratch buffer the hook keeps (test hook: one caller at a time): the list is cut every
    // 2048 edges as if those were graphs (parallel walk)
    static int* scratch_dev[16] = {nullptr}; static size_t scratch_dev_ints[16] = {0};   // (per device: the hook may be driven on several)
    int dev_id = 0;
    HIPCHECK(hipGetDevice(&dev_id));
    if (dev_id < 0 || dev_id >= 16) return fail(DBFR_ERR_ARG, "test hook: device index beyond 15");
    int*& scratch = scratch_dev[dev_id]; size_t& scratch_ints = scratch_dev_ints[dev_id];
    const int span = 2048, n_span = std::max((n_edges + span - 1) / span, 1), ccap = n_edges / 32 + n_edges / CZ_MAXSEG + n_span + 8;
    if (rf) {
      const size_t need = (size_t)n_span + 1 + 2 * (size_t)ccap;
      if (need > scratch_ints) {
        if (scratch) HIPCHECK(hipFree(scratch));           // (hipFree waits for the device: nothing in flight still reads the old buffer)
        scratch = nullptr; scratch_ints = 0;
        HIPCHECK(hipMalloc(&scratch, need * sizeof(int)));
        scratch_ints = need;
      }
      launch_flat_chunks(tgt, n_edges_dev, n_edges, span, n_span, scratch, ccap, scratch + n_span + 1, scratch + n_span + 1 + ccap, st);
    }
    ConvSite& site = job.site;   // (no chunk_segs: the hook has no segment sums, k_convz_useful walks the chunk table in front of k_convz)
    if (scratch) { site.chunk_es = scratch + n_span + 1; site.chunk_gl = scratch + n_span + 1 + ccap; site.n_chunks = scratch + n_span; }
    site.max_chunks = ccap;
    // (k_convz writes the scalar-output columns of a segment's first row only; the hook's documented layout has zeros in the other rows)
    if (rf) HIPCHECK(hipMemsetAsync(msg, 0, (size_t)n_edges * c->w.D_out * sizeof(float), st));
  }
  Ws w;
  memset(&w, 0, sizeof w);
  w.conv2 = conv2;   // dbfr_test_conv: the per-edge form; dbfr_test_conv2: the form the GEMM mode and `deep` select
  conv_group(m, w, &job, 1, deep, st);
  HIPCHECK(hipGetLastError());
  return take_launch_error();
}

// Test hook: the chunk table of DBFR_GEMM_REDUCE_FIRST for one flat, target-sorted edge list, cut every `span` edges as if those were graphs
// (graph.hip k_flat_chunk_*; the same chunk_len as the per-graph kernels of the sampler).  Device pointers; scratch = n_span + 1 ints.
// (ABI 7) Test hook: the update half of ONE denoise step on caller-supplied scores and noise slices (no score network, no workspace).
extern "C" int dbfr_test_sde_step(const dbfr_model* m, const dbfr_batch* b, const dbfr_step* step, const dbfr_scores* scores,
                                  const dbfr_noise* z, float* atom14_out, int32_t* err_word_out, void* hip_stream) {
  int rc = check_batch(m, b);
  if (rc) return rc;
  if (!step || !scores || !z || !err_word_out) return fail(DBFR_ERR_ARG, "dbfr_test_sde_step: null argument");
  if (!scores->tr || !scores->rot || !z->z_tr || !z->z_rot || (b->NTOR > 0 && (!scores->tor || !z->z_tor)) ||
      (!m->cfg.no_sc_torsion && b->NSC > 0 && (!scores->sc_tor || !z->z_sc)))
    return fail(DBFR_ERR_ARG, "dbfr_test_sde_step: null score or noise array");
  hipStream_t st = (hipStream_t)hip_stream;
  HIPCHECK(hipMemsetAsync(err_word_out, 0, sizeof(int32_t), st));
  pose_update(m, b, *step, *scores, z->z_tr, z->z_rot, z->z_tor, z->z_sc, nullptr, atom14_out, nullptr, err_word_out, st);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

extern "C" int dbfr_test_chunk_table(const int32_t* tgt, const int32_t* n_edges_dev, int32_t max_edges, int32_t span, int32_t* scratch, int32_t cap,
                                     int32_t* chunk_es, int32_t* chunk_gl, void* hip_stream) {
  if (!tgt || !n_edges_dev || !scratch || !chunk_es || !chunk_gl || span <= 0 || max_edges < 0 || cap <= 0) return fail(DBFR_ERR_ARG, "dbfr_test_chunk_table: bad argument");
  g_launch_err = false;
  const int n_span = std::max((max_edges + span - 1) / span, 1);
  launch_flat_chunks(tgt, n_edges_dev, max_edges, span, n_span, scratch, cap, chunk_es, chunk_gl, (hipStream_t)hip_stream);
  HIPCHECK(hipGetLastError());
  return take_launch_error();
}

extern "C" int dbfr_test_conv(dbfr_model* m, int32_t layer, int32_t family, int32_t n_edges, const int32_t* n_edges_dev,
                              const int32_t* tgt, const int32_t* gth, const float* emb, const float* sh,
                              const float* tab1, int32_t ld1, const int32_t* idx1, const float* tab2, int32_t ld2,
                              const int32_t* idx2, const float* x, int32_t ldx, float* msg, void* hip_stream) {
  return test_conv_impl(m, false, layer, family, n_edges, n_edges_dev, tgt, gth, emb, sh, tab1, ld1, idx1, tab2, ld2, idx2, x, ldx,
                        msg, hip_stream);
}

extern "C" int dbfr_test_conv2(dbfr_model* m, int32_t layer, int32_t family, int32_t n_edges, const int32_t* n_edges_dev,
                               const int32_t* tgt, const int32_t* gth, const float* emb, const float* sh,
                               const float* tab1, int32_t ld1, const int32_t* idx1, const float* tab2, int32_t ld2,
                               const int32_t* idx2, const float* x, int32_t ldx, float* msg, void* hip_stream) {
  return test_conv_impl(m, true, layer, family, n_edges, n_edges_dev, tgt, gth, emb, sh, tab1, ld1, idx1, tab2, ld2, idx2, x, ldx,
                        msg, hip_stream);
}

// (ABI 6) ... with the message interface of DBFR_GEMM_REDUCE_FIRST: seg_first[e] = 1 marks the rows whose scalar-output columns hold a segment's sum (the
// other rows' scalar columns are not read -- they may hold anything), the vector columns are per edge; seg_first == NULL: every column of every row
extern "C" int dbfr_test_reduce_ln2(dbfr_model* m, int32_t layer, int32_t family, const float* msg, const int32_t* row_start, const int32_t* row_cnt,
                                    int32_t n_nodes, const float* old, int32_t d_old, float* out, int32_t mode, const uint8_t* seg_first, void* hip_stream) {
  if (!m) return fail(DBFR_ERR_ARG, "null model");
  const ModelConv* c = pick_conv(m, layer, family);
  if (!c) return fail(DBFR_ERR_ARG, "no such conv");
  unsigned long long lanes = 0;
  if (seg_first) {
    if (!c->k144) return fail(DBFR_ERR_ARG, "dbfr_test_reduce_ln2: seg_first with a conv that has no reduce-first form");
    lanes = convz_sc_lanes(c->z);
  }
  launch_reduce_ln(msg, row_start, row_cnt, n_nodes, c->w.D_out, c->w.ln, old, d_old, out, c->w.D_out, mode, (hipStream_t)hip_stream, seg_first, lanes);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

extern "C" int dbfr_test_reduce_ln(dbfr_model* m, int32_t layer, int32_t family, const float* msg,
                                   const int32_t* row_start, const int32_t* row_cnt, int32_t n_nodes, const float* old,
                                   int32_t d_old, float* out, int32_t mode, void* hip_stream) {
  if (!m) return fail(DBFR_ERR_ARG, "null model");
  const ModelConv* c = pick_conv(m, layer, family);
  if (!c) return fail(DBFR_ERR_ARG, "no such conv");
  launch_reduce_ln(msg, row_start, row_cnt, n_nodes, c->w.D_out, c->w.ln, old, d_old, out, c->w.D_out, mode,
                   (hipStream_t)hip_stream);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

// ------------------------------------------------------------------------------------------------
// (ABI 8) Test hooks: the small kernels of the score network alone -- each runs the launcher run_score calls, with the model's own packed weights and
// tables, on caller-supplied device buffers; nothing is synchronised.
extern "C" int dbfr_test_time_embed(const dbfr_model* m, const float* t, int32_t G, float* temb_out, void* hip_stream) {
  if (!m || !t || !temb_out || G <= 0) return fail(DBFR_ERR_ARG, "dbfr_test_time_embed: null argument");
  launch_time_embed(t, G, m->cfg.emb_scale, temb_out, (hipStream_t)hip_stream);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

extern "C" int dbfr_test_mlp(const dbfr_model* m, int32_t which, int32_t n_rows_max, const int32_t* n_rows_dev, const float* temb,
                             const int32_t* row_graph_tab, const int32_t* tgt, const int32_t* aux, const float* dist, const float* bond_feat,
                             const float* lig_node, float* out, void* hip_stream) {
  if (!m || !out) return fail(DBFR_ERR_ARG, "dbfr_test_mlp: null argument");
  // the weight set, the input mode and the Gaussian tables run_score pairs with it
  struct { const Mlp2* w; int mode; const float *off, *c; } sets[7] = {
      {&m->lig_node_emb, IN_LIGNODE, nullptr, nullptr},
      {&m->lig_edge_emb, IN_LIGEDGE, m->gs_lig_off, m->gs_lig_c},
      {&m->atom_edge_emb, IN_TG, m->gs_atom_off, m->gs_atom_c},
      {&m->la_edge_emb, IN_TG, m->gs_cross_off, m->gs_cross_c},
      {&m->center_edge_emb, IN_TG, m->gs_center_off, m->gs_center_c},
      {&m->tor_edge_emb, IN_G, m->gs_lig_off, m->gs_lig_c},
      {&m->sc_edge_emb, IN_G, m->gs_atom_off, m->gs_atom_c}};
  if (which < 0 || which >= 7 || (which == DBFR_MLP_SC_EDGE && m->cfg.no_sc_torsion)) return fail(DBFR_ERR_ARG, "dbfr_test_mlp: no such weight set");
  const int mode = sets[which].mode;
  if (n_rows_max < 0) return fail(DBFR_ERR_ARG, "dbfr_test_mlp: negative row capacity");
  if (mode != IN_G && (!temb || !row_graph_tab)) return fail(DBFR_ERR_ARG, "dbfr_test_mlp: null time embedding or batch vector");
  if (mode != IN_LIGNODE && !dist) return fail(DBFR_ERR_ARG, "dbfr_test_mlp: null distances");
  if (mode == IN_LIGEDGE && (!aux || !bond_feat)) return fail(DBFR_ERR_ARG, "dbfr_test_mlp: null bond index or bond features");
  if (mode == IN_LIGNODE && !lig_node) return fail(DBFR_ERR_ARG, "dbfr_test_mlp: null ligand node features");
  MlpArgs a; memset(&a, 0, sizeof a);
  a.w = *sets[which].w; a.mode = mode; a.n_rows_dev = n_rows_dev; a.n_rows_max = n_rows_max; a.temb = temb; a.row_graph_tab = row_graph_tab;
  a.tgt = tgt; a.aux = aux; a.dist = dist; a.bond_feat = bond_feat; a.nfeat = m->cfg.lig_edge_features;
  a.lig_node = lig_node; a.nnode = m->cfg.lig_node_features;
  a.gs_offset = sets[which].off; a.gs_coeff = sets[which].c; a.out = out;
  launch_mlp(a, (hipStream_t)hip_stream);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

extern "C" int dbfr_test_atom_encoder(const dbfr_model* m, const float* pocket_feat, const int32_t* atm_batch, const float* temb, int32_t NA,
                                      float* out, void* hip_stream) {
  if (!m || !pocket_feat || !atm_batch || !temb || !out || NA < 0) return fail(DBFR_ERR_ARG, "dbfr_test_atom_encoder: null argument");
  AtomEncArgs a; a.pocket_feat = pocket_feat; a.atm_batch = atm_batch; a.temb = temb;
  for (int i = 0; i < 5; ++i) { a.emb[i] = m->atom_emb[i]; a.dims[i] = m->atom_dims[i]; }
  a.lin_t = m->atom_lin_t; a.NA = NA; a.out = out;
  launch_atom_encoder(a, (hipStream_t)hip_stream);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

extern "C" int dbfr_test_reduce_ln_layer(const dbfr_model* m, int32_t layer, const float* const* msg, const int32_t* const* row_start,
                                         const int32_t* const* row_cnt, const uint8_t* const* seg_first, int32_t NL, int32_t NA, const float* old_l,
                                         const float* old_a, float* out_l, float* out_a, void* hip_stream) {
  if (!m || !msg || !row_start || !row_cnt || !old_l || !old_a || !out_l || !out_a) return fail(DBFR_ERR_ARG, "dbfr_test_reduce_ln_layer: null argument");
  if (layer < 0 || layer >= m->cfg.num_conv_layers || NL < 0 || NA < 0) return fail(DBFR_ERR_ARG, "dbfr_test_reduce_ln_layer: no such layer");
  ReduceLayerArgs ra;
  for (int i = 0; i < 4; ++i) {
    if (!msg[i] || !row_start[i] || !row_cnt[i] || (seg_first && !seg_first[i])) return fail(DBFR_ERR_ARG, "dbfr_test_reduce_ln_layer: null edge-set argument");
    ra.msg[i] = msg[i]; ra.row_start[i] = row_start[i]; ra.row_cnt[i] = row_cnt[i]; ra.ln[i] = m->layer[layer][i].w.ln;
    ra.first[i] = seg_first ? seg_first[i] : nullptr; ra.sc_lanes[i] = seg_first ? convz_sc_lanes(m->layer[layer][i].z) : 0;
  }
  ra.NL = NL; ra.NA = NA; ra.D = m->layer[layer][0].w.D_out; ra.D_old = m->layer[layer][0].w.D_in;
  ra.old_l = old_l; ra.old_a = old_a; ra.out_l = out_l; ra.out_a = out_a;
  launch_reduce_ln_layer(ra, (hipStream_t)hip_stream);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

extern "C" int dbfr_test_center_edges(const dbfr_batch* b, int32_t* tgt, int32_t* gth, float* dist, float* sh, int32_t* row_start, int32_t* row_cnt,
                                      void* hip_stream) {
  if (!b || !tgt || !gth || !dist || !sh || !row_start || !row_cnt || !b->lig_ptr || !b->lig_pos || b->G <= 0)
    return fail(DBFR_ERR_ARG, "dbfr_test_center_edges: null argument");
  launch_center_edges(*b, tgt, gth, dist, sh, row_start, row_cnt, (hipStream_t)hip_stream);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

extern "C" int dbfr_test_trrot(const dbfr_model* m, const float* gp, const float* temb, const float* tr_sigma, const float* rot_norm, int32_t G,
                               float* tr_out, float* rot_out, int32_t* err_word, void* hip_stream) {
  if (!m || !gp || !temb || !tr_sigma || !rot_norm || !tr_out || !rot_out || !err_word || G <= 0) return fail(DBFR_ERR_ARG, "dbfr_test_trrot: null argument");
  TrRotArgs a; a.gp = gp; a.temb = temb; a.tr_sigma = tr_sigma; a.rot_norm = rot_norm;
  a.tr = m->tr_final; a.rot = m->rot_final; a.G = G; a.scale_by_sigma = m->cfg.scale_by_sigma; a.tr_out = tr_out;
  a.rot_out = rot_out; a.err = err_word;
  launch_trrot(a, (hipStream_t)hip_stream);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

extern "C" int dbfr_test_bond_attr(const dbfr_model* m, int32_t which, const float* nodes, int32_t ld, const int32_t* b0, const int32_t* b1,
                                   const int32_t* bsel, int32_t n, float* attr_out, void* hip_stream) {
  if (!m || !nodes || !b0 || !attr_out || n < 0 || ld < NS) return fail(DBFR_ERR_ARG, "dbfr_test_bond_attr: null argument");
  if (which == DBFR_TOR_LIGAND) {
    if (!b1 || !bsel) return fail(DBFR_ERR_ARG, "dbfr_test_bond_attr: the ligand head needs bond_dst and tor_bond");
    launch_bond_attr(nodes, ld, b0, b1, bsel, 0, n, attr_out, (hipStream_t)hip_stream);
  } else if (which == DBFR_TOR_SIDECHAIN) {
    launch_bond_attr(nodes, ld, b0, nullptr, nullptr, 2, n, attr_out, (hipStream_t)hip_stream);
  } else return fail(DBFR_ERR_ARG, "dbfr_test_bond_attr: no such head");
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}

extern "C" int dbfr_test_tor_final(const dbfr_model* m, int32_t which, const float* feat, const float* norm2, int32_t n, float* out, void* hip_stream) {
  if (!m || !feat || !norm2 || !out || n < 0) return fail(DBFR_ERR_ARG, "dbfr_test_tor_final: null argument");
  if (which != DBFR_TOR_LIGAND && (which != DBFR_TOR_SIDECHAIN || m->cfg.no_sc_torsion)) return fail(DBFR_ERR_ARG, "dbfr_test_tor_final: no such head");
  launch_tor_final(feat, which == DBFR_TOR_LIGAND ? m->tor_final : m->sc_final, norm2, m->cfg.scale_by_sigma, n, out, (hipStream_t)hip_stream);
  HIPCHECK(hipGetLastError());
  return DBFR_OK;
}
