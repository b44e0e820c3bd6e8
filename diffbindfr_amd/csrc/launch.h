// The score network's kernel interface: the argument structs and launchers of conv.hip, conv2.hip, conv2h.hip, convz.hip, graph.hip and
// heads.hip, declared ONCE.  api.cpp (the caller) and the six kernel files (the definitions) all include this header, so the struct the
// host fills is the struct the kernel reads, and the library is linked with -z defs: a definition that drifts from its prototype here is
// an unresolved symbol at build time, not a wrong call at run time.
#pragma once
#include "common.h"

// per-graph limits (dbfr_batch max_nl / max_na, checked by check_batch in api.cpp)
#define MAX_NL 256      // per-graph ligand atoms (the ligand kernels of heads.hip keep a conformer in static LDS)
#define MAX_NA 8192     // per-graph pocket atoms: the graph's coordinates are staged in dynamic LDS sized by the batch's
                        // largest graph (16 B per atom, 128 KB of the CU's 160 KB at the limit)

// ---- conv.hip / conv2.hip / conv2h.hip / convz.hip
void launch_conv(const ConvArgs& a, hipStream_t st);
void launch_conv_layer(const ConvArgs* c4, hipStream_t st);
void launch_conv2(const Conv2Args& a, hipStream_t st);
void launch_conv2h(const Conv2Args& a, hipStream_t st);
void launch_convz(const ConvZArgs& a, hipStream_t st, bool useful_pass = false);   // useful_pass: k_convz_useful in front (callers without the edge set's segment sum)
void launch_reduce_ln(const float* msg, const int* row_start, const int* row_cnt, int N, int D, const LNDesc& ln,
                      const float* old, int D_old, float* out, int ldo, int mode, hipStream_t st, const uint8_t* first = nullptr, unsigned long long sc_lanes = 0);
struct ReduceLayerArgs {
  const float* msg[4]; const int* row_start[4]; const int* row_cnt[4]; LNDesc ln[4];   // ll, al, aa, la
  int NL, NA, D, D_old;
  const float* old_l; const float* old_a; float* out_l; float* out_a;
  const uint8_t* first[4]; unsigned long long sc_lanes[4];   // DBFR_GEMM_REDUCE_FIRST: the segment-start flags of the four edge sets and the lanes of scalar-output columns (row_sum:
                                                              // those columns are read from a segment's first row only), else null / 0
};
void launch_reduce_ln_layer(const ReduceLayerArgs& a, hipStream_t st);

// ---- graph.hip
enum SetKind { SET_LL = 0, SET_AA = 1, SET_AL = 2, SET_LA = 3, SET_TOR = 4, SET_SC = 5, N_SETS = 6 };

struct GraphArgs {
  dbfr_batch b;
  const int* lig_batch;   // [NL]
  const int* atm_batch;   // [NA]
  const uint8_t* is_cab;  // [NA]
  const int* n_cab;       // [G]
  const float* tr_sigma;  // [G]
  float lig_cut2, atom_cut2, cross_cut2;
  int lig_cap, atom_cap, dynamic_cross;
  EdgeSet set[N_SETS];
  int* err;               // device status block: [0] status bits, [1] first step (+1) whose edge lists overflowed,
                          // [2+k] set k overflowed in THIS step, [8+k] largest edge count seen for set k
  int step;               // sampler step index (0 for dbfr_score)
  int lds_nl, lds_na;     // LDS staging capacities (>= max_nl / max_na of the batch)
  int n_chunk;            // EDGE_CHUNK-target chunks per graph every set is split into (own workgroup each)
  int lanes;              // lanes per target of the edge builder (1 | 4); n_chunk and lanes are chosen ONCE per call (dbfr_edge_form) and
                          // shared by every launcher below: the g_cnt / g_base layout depends on both
  long long* chunk_segs;  // profiling, else null: [N_SETS] per edge set the summed segment counts of this step's chunks (k_graph_chunks clears them,
                          // k_chunk_fill adds).  With the set's edge count -- every edge lies in exactly one chunk -- that is what the profile counters of
                          // every k_convz launch on the set are linear in
};
void dbfr_edge_form(const dbfr_batch& b, int* n_chunk, int* lanes);
void launch_edges(const GraphArgs& A, bool heads_only, hipStream_t st);
void launch_edge_log(const GraphArgs& A, int* log_row, int stride, hipStream_t st);
void launch_edge_ties(const GraphArgs& A, int* log_row, int stride, float tol, hipStream_t st);
void launch_graph_chunks(const GraphArgs& A, hipStream_t st);
void launch_flat_chunks(const int* tgt, const int* n_edges, int max_edges, int span, int n_span, int* cnt0, int cap, int* chunk_es, int* chunk_gl, hipStream_t st);
void launch_row_absmax(const float* lx, const int* lig_ptr, float* out_l, const float* ax, const int* atm_ptr, float* out_a, int ld, int D, int G, int n_rows_a, hipStream_t st);
void launch_batch_vectors(const dbfr_batch& b, int* lig_batch, int* atm_batch, uint8_t* is_cab, int* n_cab,
                          int* tor_batch, int* sc_batch, hipStream_t st);
void launch_time_embed(const float* t, int G, float emb_scale, float* temb, hipStream_t st);

enum MlpIn { IN_LIGNODE = 0, IN_LIGEDGE = 1, IN_TG = 2, IN_G = 3 };   // input assembly of k_mlp (graph.hip)

struct MlpArgs {
  Mlp2 w;
  int mode;
  const int* n_rows_dev;   // device row count (edges) or null
  int n_rows_max;
  const float* temb;       // [G][EMB]
  const int* row_graph_tab;  // batch vector indexed by tgt (edges) or by row (nodes)
  const int* tgt;          // per-edge target (graph lookup) or null
  const int* aux;          // bond index per edge (IN_LIGEDGE)
  const float* dist;       // per-edge distance
  const float* bond_feat;  // [EB][nfeat]
  int nfeat;
  const float* lig_node;   // [NL][nfeat_node]
  int nnode;
  const float* gs_offset;  // [EMB] GaussianSmearing buffers
  const float* gs_coeff;   // [1]
  float* out;              // [rows][NS]
};
void launch_mlp(const MlpArgs& a, hipStream_t st);

struct AtomEncArgs {
  const float* pocket_feat;  // [NA][5]
  const int* atm_batch;
  const float* temb;
  const float* emb[5];       // [dim_i][NS]
  int dims[5];
  const float* lin_t;        // [NS+EMB][NS] transposed scalar_lin.weight
  int NA;
  float* out;                // [NA][NS]
};
void launch_atom_encoder(const AtomEncArgs& a, hipStream_t st);

// ---- heads.hip
void launch_center_edges(const dbfr_batch& b, int* tgt, int* gth, float* dist, float* sh, int* row_start, int* row_cnt,
                         hipStream_t st);
struct TrRotArgs {
  const float* gp; const float* temb; const float* tr_sigma; const float* rot_norm;
  Mlp2 tr, rot; int G; int scale_by_sigma; float* tr_out; float* rot_out; int* err;
};
void launch_trrot(const TrRotArgs& a, hipStream_t st);
void launch_bond_attr(const float* x, int ldx, const int* b0, const int* b1, const int* bsel, int stride, int n,
                      float* out, hipStream_t st);
void launch_tor_final(const float* feat, const Mlp2& w, const float* norm2, int scale, int n, float* out, hipStream_t st);
struct SdeLigArgs {
  dbfr_batch b;
  const float* tr_score; const float* rot_score; const float* tor_score;
  const float* z_tr; const float* z_rot; const float* z_tor;     // this step's slices
  float dt, tr_g2, tr_gsdt, rot_g2, rot_gsdt, tor_g2, tor_gsdt;
  float* traj;   // [NL,3] slice or null
  int* err;
};
void launch_sde_ligand(const SdeLigArgs& a, hipStream_t st);
void launch_sidechain(const dbfr_batch& b, const float* score, const float* z, float dt, float g2, float gsdt,
                      const int* a14_group, float* atom14_out, float* traj14, const int* err, hipStream_t st);
void launch_fill(float* p, float v, int n, hipStream_t st);
void launch_set_int(int* p, int v, hipStream_t st);
void launch_init_poses(const dbfr_batch& b, const dbfr_init_tape& z, const int* a14_group, float* atom14_out, hipStream_t st);
void launch_extract_templates(int n_res, const int* aatype, const float* pos14, float* transl, float* rots, float* frames,
                              float* rigid, float* angle, hipStream_t st);
void launch_select_pocket(int n_prot, int n_res_total, const int* res_ptr, int m, const float* pos, const float* mask, const int* ref_ptr,
                          const float* ref, float cut2, int max_neighbors, float* d2, unsigned char* out, hipStream_t st);
#define ACC_BATCH_MAX 48
struct AccBatch { const void* n[ACC_BATCH_MAX]; double coef[ACC_BATCH_MAX]; double* dst[ACC_BATCH_MAX]; unsigned long long wide; int count; };   // up to 48 counter
                          // updates of one k_acc_batch launch: dst += coef * *n, n an int, or a long long where the update's bit of `wide` is set
void launch_acc_batch(const AccBatch& b, hipStream_t st);
