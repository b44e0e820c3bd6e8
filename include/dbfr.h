/*
 * dbfr.h -- C ABI of the MI355X-native DiffBindFR reverse-diffusion sampler.
 *
 * The reference (HBioquant/DiffBindFR) is 100% Python: it has no FFI for this
 * path.  Its operator boundary is the mmcv-style registry + nn.Module contract
 *   INTERACTION['TensorProductModel']   druglib/models/Docking/interaction/tpscore.py:202-573
 *   MLDOCK_BUILDER['DiffBindFR']        druglib/models/Docking/scFlex.py:26-250
 * (druglib/models/builder.py:7-34).  This header is the C ABI underneath the
 * Python classes that plug into those registries (diffbindfr_amd/score_model.py,
 * diffbindfr_amd/sampler.py); INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / hip types in signatures
 *     (a hipStream_t travels as void*; NULL = the null stream);
 *   - every entry point returns 0 on success or a negative dbfr_status;
 *     dbfr_last_error() gives the message of the last failure on this thread;
 *   - "host" pointers are read during the call and not retained; "device"
 *     pointers must stay valid until the stream work that uses them is done;
 *   - one model handle per device; a handle is thread-compatible, not thread-safe;
 *   - all arithmetic is fp32 (the reference runs fp32: base.py:22 fp16 off);
 *     indices are int32 on the device side.
 */
#ifndef DBFR_H
#define DBFR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DBFR_ABI_VERSION 9   /* 2: + dbfr_sample_range, dbfr_capacity_report, dbfr_sdf_*, dbfr_mdn_*, dbfr_build_id, dbfr_test_conv2;
                                3: + dbfr_model_set_edge_log, dbfr_model_fallback_convs, dbfr_test_pack_f16_depth, dbfr_probe_mfma_f16 (additions only);
                                4: + DBFR_GEMM_REDUCE_FIRST (the new default), dbfr_profile_executed_flops; dbfr_model_set_edge_log takes the graph capacity; DBFR_GEMM_SPLIT_BF16_L1 (k_conv2s) retired; dbfr_test_conv2's message rows in that mode hold segment sums;
                                5: + dbfr_model_rowscaled_convs (per-row factors instead of the three-bf16-piece fall-back), dbfr_test_pack_f16_rows, dbfr_test_chunk_table; the reduce-first chunks hold <= 4 targets; DBFR_GEMM_SPLIT_BF16 (k_conv2r) retired;
                                6: + dbfr_profile_useful_flops, dbfr_model_set_tie_log, dbfr_test_reduce_ln2; dbfr_model_set_edge_log accepts batches with fewer graphs than its capacity; an unknown DBFR_GEMM value fails dbfr_model_create;
                                   later additions under the same number: dbfr_vina_in, dbfr_vina_opts, dbfr_vina_workspace_bytes, dbfr_vina_score, dbfr_vina_score_at, dbfr_vina_minimize, dbfr_vina_flex_in, dbfr_vina_flex_workspace_bytes, dbfr_vina_flex_score_at, dbfr_vina_flex_minimize,
                                   dbfr_pose_rmsd_in, dbfr_modes_opts, dbfr_pose_rmsd_matrix, dbfr_select_modes,
                                   dbfr_pose_check_in, dbfr_pose_check_opts, dbfr_pose_check_out, dbfr_pose_check,
                                   dbfr_xtc_in, dbfr_xtc_opts, dbfr_xtc_workspace_bytes, dbfr_xtc_encode, dbfr_pdb_atom_map,
                                   dbfr_pdb_ligand, dbfr_complex_pdb_format, dbfr_complex_pdb_write_files,
                                   dbfr_sites_opts, dbfr_sites_in, dbfr_sites_out, dbfr_sites_workspace_bytes, dbfr_find_sites;
                                7: + dbfr_test_sde_step (additions only);
                                   later additions under the same number: dbfr_interactions_in, dbfr_interactions_opts, dbfr_interactions_out,
                                   dbfr_interactions, dbfr_pocket_check_in, dbfr_pocket_check_opts, dbfr_pocket_check_out,
                                   dbfr_pocket_check, dbfr_sasa_in, dbfr_sasa_opts, dbfr_sasa_out, dbfr_sasa, dbfr_seq_align,
                                   dbfr_holo_site_in, dbfr_holo_site, dbfr_holo_metrics_in, dbfr_holo_metrics_opts, dbfr_holo_metrics_out,
                                   dbfr_holo_metrics, dbfr_hetero_check_in, dbfr_hetero_check_opts, dbfr_hetero_check_out,
                                   dbfr_hetero_check, dbfr_hydrogens_in, dbfr_hydrogens_opts, dbfr_hydrogens_out, dbfr_hydrogens,
                                   dbfr_vina_decompose_in, dbfr_vina_decompose_opts, dbfr_vina_decompose_out, dbfr_vina_decompose; XS type code 17 (Met_D) in dbfr_vina_in;
                                8: + dbfr_test_time_embed, dbfr_test_mlp, dbfr_test_atom_encoder, dbfr_test_reduce_ln_layer, dbfr_test_center_edges, dbfr_test_trrot, dbfr_test_bond_attr, dbfr_test_tor_final (additions only);
                                   later additions under the same number: dbfr_vina_search_opts, dbfr_vina_search_workspace_bytes, dbfr_vina_search,
                                   dbfr_test_philox4x32, dbfr_test_vina_mutation,
                                   dbfr_vina_flex_search_workspace_bytes, dbfr_vina_flex_search,
                                   dbfr_test_pack_conv,
                                   dbfr_cavity_in, dbfr_cavity_opts, dbfr_cavity_out, dbfr_pose_cavity_workspace_bytes, dbfr_pose_cavity,
                                   dbfr_pocket_states_in, dbfr_pocket_states_opts, dbfr_pocket_states_out, dbfr_pocket_states,
                                   dbfr_shape_in, dbfr_shape_opts, dbfr_shape_out, dbfr_shape_overlap;
                                9: + dbfr_mdn_seg, dbfr_mdn_vseg, dbfr_test_mdn_lin, dbfr_test_mdn_gt_attn, dbfr_test_mdn_gvp, dbfr_test_mdn_gvp_ln, dbfr_test_mdn_mean_in, dbfr_test_mdn_seq_concat, dbfr_test_mdn_gt_layer, dbfr_test_mdn_head (additions only) */

typedef enum {
  DBFR_OK = 0,
  DBFR_ERR_ARG = -1,       /* bad argument / unsupported configuration            */
  DBFR_ERR_HIP = -2,       /* a HIP runtime call failed                           */
  DBFR_ERR_CAPACITY = -3,  /* workspace edge capacity exceeded (see dbfr_limits)  */
  DBFR_ERR_SELFTEST = -4,  /* built-in Clebsch-Gordan closed forms failed self-check */
  DBFR_ERR_NUMERIC = -5    /* non-finite score / Kabsch determinant check failed  */
} dbfr_status;

typedef struct dbfr_model dbfr_model; /* packed weights resident in HBM */

/* ---- model hyper-parameters (DiffBindFR/configs/diffbindfr_ts.py:107-142).
 * Only the reference's inference configuration family is supported:
 * ns=48, nv=12, sh_lmax=2, 32-d embeddings, use_second_order_repr=False.      */
typedef struct {
  int32_t ns, nv, sh_lmax;
  int32_t num_conv_layers;
  int32_t lig_node_features, lig_edge_features;
  int32_t distance_embed_dim, sigma_embed_dim;
  float   emb_scale;
  float   lig_cutoff, atom_cutoff, cross_cutoff, center_max_distance;
  int32_t atom_max_neighbors;  /* radius_graph cap for the pocket graph (1000)   */
  int32_t lig_max_neighbors;   /* torch_cluster default cap (32), tpscore.py:586 */
  int32_t dynamic_max_cross;   /* 1: cross cutoff = 0.2*tr_sigma + 5             */
  int32_t scale_by_sigma;
  int32_t no_sc_torsion;
} dbfr_model_cfg;

/* One named fp32 tensor of the reference state_dict (host memory, row-major,
 * exactly the shape the reference module holds; names relative to
 * TensorProductModel, e.g. "lig_conv_layers.3.fc.lin.3.weight").               */
typedef struct {
  const char*  name;
  const float* data;
  int64_t      numel;
} dbfr_tensor;

/* Builds the device-resident packed model (radial-MLP weights re-tiled into
 * MFMA fragment order with the tensor-product path normalisation folded in).
 * Replaces: TensorProductModel.__init__ + load_checkpoint(strict=True)
 * (tpscore.py:215-410; DiffBindFR/common/engines.py:137-165).  Every tensor of
 * SURVEY.md Appendix B.3 must be present; unknown names are an error.          */
int dbfr_model_create(const dbfr_model_cfg* cfg, const dbfr_tensor* tensors, int32_t n_tensors,
                      dbfr_model** out);
void dbfr_model_destroy(dbfr_model* m);

/* ---- one collated batch of G graphs (complex x pose), device pointers.
 * Layout = the reference's batched dict with int32
 * indices, CSR pointers instead of batch vectors, and the ragged python lists
 * flattened.  Tensors marked in/out are advanced in place by dbfr_sample.       */
typedef struct {
  int32_t G;        /* graphs                                                    */
  int32_t NL;       /* ligand heavy atoms, all graphs                            */
  int32_t NA;       /* pocket heavy atoms, all graphs                            */
  int32_t NR;       /* pocket residues, all graphs                               */
  int32_t EB;       /* directed ligand bonds (both directions), sorted by src    */
  int32_t NTOR;     /* ligand rotatable bonds (tor_edge_mask.sum())              */
  int32_t NSC;      /* side-chain torsions (sc_torsion_edge_mask.sum())          */
  int32_t max_nl, max_na, max_nr; /* per-graph maxima (host-known)               */
  /* ligand */
  const int32_t* lig_ptr;     /* [G+1]                                           */
  const float*   lig_node;    /* [NL, lig_node_features]                         */
  float*         lig_pos;     /* [NL,3]                               in/out     */
  const int32_t* bond_src;    /* [EB] global ligand atom index                   */
  const int32_t* bond_dst;    /* [EB]                                            */
  const float*   bond_feat;   /* [EB, lig_edge_features]                         */
  const int32_t* bond_ptr;    /* [NL+1] CSR of bonds by bond_src                 */
  const int32_t* tor_ptr;     /* [G+1]  torsions per graph                       */
  const int32_t* tor_bond;    /* [NTOR] index into bond_* (masked bonds, in order) */
  const uint8_t* rot_mask;    /* rot_node_mask rows, one byte per ligand atom    */
  const int64_t* rot_mask_off;/* [NTOR] byte offset of each row in rot_mask      */
  /* pocket */
  const int32_t* atm_ptr;     /* [G+1]                                           */
  const int32_t* res_ptr;     /* [G+1]                                           */
  const float*   pocket_feat; /* [NA,5] (atom37, coarse22, element4, aatype, is_backbone) */
  float*         rec_pos;     /* [NA,3]                               in/out     */
  const int32_t* sequence;    /* [NR]                                            */
  const float*   backbone_transl; /* [NR,3]                                      */
  const float*   backbone_rots;   /* [NR,3,3]                                    */
  const float*   default_frame;   /* [NR,8,4,4]                                  */
  const float*   rigid_group_positions; /* [NR,14,3]                             */
  float*         torsion_angle;   /* [NR,5] (psi, chi1..4) radians    in/out     */
  const int32_t* atom14_slot;     /* [NR,14] compact atom index or -1 (atom14_mask) */
  const int32_t* sc_res_chi;      /* [NSC] res*4+k of each masked chi, row-major */
  const int32_t* sc_bond;         /* [NSC,2] global atom ids (j,k) of the chi bond */
  const int32_t* sc_ptr;          /* [G+1] side-chain torsions per graph         */
} dbfr_batch;

/* Capacity knobs of the per-step edge lists (graphs are rebuilt every step).    */
typedef struct {
  int32_t aa_avg_neighbors;     /* pocket graph: mean edges per atom budgeted (default 24)   */
  int32_t cross_avg_neighbors;  /* non-CA/CB pocket atoms per ligand atom budgeted (default 64) */
} dbfr_limits;

/* Bytes of device workspace dbfr_score/dbfr_sample need for this batch shape.   */
int dbfr_workspace_bytes(const dbfr_model* m, const dbfr_batch* b, const dbfr_limits* lim, size_t* bytes);

/* ---- level 1: one score-network evaluation.
 * Replaces TensorProductModel.forward (tpscore.py:462-573).  Per-graph /
 * per-torsion conditioning arrives as device arrays exactly as set_time
 * produces it (scFlex.py:104-122).  Outputs are device arrays.                  */
typedef struct {
  const float* t;                 /* [G]                                          */
  const float* tr_sigma;          /* [G]                                          */
  const float* rot_score_norm;    /* [G]                                          */
  const float* tor_score_norm2;   /* [NTOR]                                       */
  const float* sc_tor_score_norm2;/* [NSC] (already masked/compacted)             */
} dbfr_cond;

typedef struct {
  float* tr;      /* [G,3]  */
  float* rot;     /* [G,3]  */
  float* tor;     /* [NTOR] */
  float* sc_tor;  /* [NSC]  */
} dbfr_scores;

int dbfr_score(dbfr_model* m, const dbfr_batch* b, const dbfr_cond* cond, const dbfr_scores* out,
               void* workspace, size_t workspace_bytes, const dbfr_limits* lim, void* hip_stream);

/* ---- level 2: the whole reverse-SDE sampler.
 * Replaces DiffBindFR.sample (scFlex.py:124-250): `n_steps` Euler-Maruyama steps
 * { set_time -> score net -> perturbations -> ligand rigid+torsion update + Kabsch
 *   -> chi update + side-chain rebuild }, entirely on the device.
 * Per-step scalars come from the host schedule (diffbindfr_amd/schedule.py mirrors
 * scFlex.py:83-122,154-161); the N(0,1) tape is supplied by the caller (device).  */
typedef struct {
  float t, dt;
  float tr_sigma, rot_score_norm, tor_score_norm2;   /* conditioning (uniform over graphs) */
  float tr_g2, tr_gsdt;      /* g^2 and g*sqrt(dt) as the reference's fp32 ops yield them */
  float rot_g2, rot_gsdt;
  float tor_g2, tor_gsdt;
  float sc_g2, sc_gsdt;
} dbfr_step;

typedef struct {
  const float* z_tr;   /* [n_steps, G, 3]  */
  const float* z_rot;  /* [n_steps, G, 3]  */
  const float* z_tor;  /* [n_steps, NTOR]  */
  const float* z_sc;   /* [n_steps, NSC]   */
} dbfr_noise;

/* atom14_out: [NR,14,3] device, masked atom14 positions after the last step
 * (may be NULL).  traj_lig / traj_atom14: optional [n_steps,...] device buffers
 * receiving every step (visualize=True), else NULL.                              */
int dbfr_sample(dbfr_model* m, const dbfr_batch* b, const dbfr_step* steps, int32_t n_steps,
                const dbfr_noise* noise, float* atom14_out, float* traj_lig, float* traj_atom14,
                void* workspace, size_t workspace_bytes, const dbfr_limits* lim, void* hip_stream);

/* The same, steps [step_begin, n_steps) only: `steps`, `noise` and the trajectory buffers are indexed by the absolute
 * step.  Used to RESUME after DBFR_ERR_CAPACITY: once an edge list of step s does not fit, that set is left empty,
 * the pose updates of step s and of every later step are skipped (the state stays as it was at the beginning of step
 * s) and the device remembers s and the edge counts it needed.  The caller reads them with dbfr_capacity_report,
 * raises dbfr_limits, sizes a new workspace and calls dbfr_sample_range(step_begin = s).                           */
int dbfr_sample_range(dbfr_model* m, const dbfr_batch* b, const dbfr_step* steps, int32_t n_steps, int32_t step_begin,
                      const dbfr_noise* noise, float* atom14_out, float* traj_lig, float* traj_atom14,
                      void* workspace, size_t workspace_bytes, const dbfr_limits* lim, void* hip_stream);

/* After dbfr_status_sync returned DBFR_ERR_CAPACITY: the first step whose edge lists overflowed (-1: none) and the
 * largest edge count each set needed so far, [8] int64 in dbfr_status_sync's counter order
 * {lig, atom, cross lig<-atom, 0, tor, sc_tor, cross atom<-lig, 0}.  Synchronises the stream.                      */
int dbfr_capacity_report(void* workspace, void* hip_stream, int32_t* first_failed_step, int64_t* needed_edges);

/* Per-graph read-out of the per-step graphs (dbfr_status_sync's counters are per batch).  With log != NULL every step s < n_steps_cap of
 * the dbfr_sample / dbfr_sample_range calls that follow on this model writes the edge count of graph g in edge set k to
 * log[(s * 6 + k) * n_graphs_cap + g] (device int32, caller-owned, n_steps_cap * 6 * n_graphs_cap entries; a batch with MORE graphs than
 * n_graphs_cap is refused with DBFR_ERR_ARG before anything is launched, a smaller one -- the ragged last batch of a sharded run -- fills the
 * first G entries of each row; until ABI 6 any other count was refused, and only after the step's first launches), k = {0 ligand
 * (bonds + radius_graph, tpscore.py:586), 1 pocket (:613), 2 cross lig<-atom, 3 cross atom<-lig (the same pairs, :655-660), 4 ligand
 * torsion (:721), 5 side-chain torsion (:747)}; dbfr_score writes row s = 0.  A set that overflowed its capacity still reports the count
 * it needed.  log == NULL switches the read-out off (the default).  The counts make a hard-cutoff event visible: two runs whose
 * coordinates differ in the 5th decimal build different graphs exactly where a pair sits within rounding distance of a cutoff
 * (tests/test_examples.py).                                                                                                        */
int dbfr_model_set_edge_log(dbfr_model* m, int32_t* log_dev, int32_t n_steps_cap, int32_t n_graphs_cap);
/* (ABI 6) The companion read-out: ties[(s * 6 + k) * n_graphs_cap + g] = the number of candidate pairs of graph g in edge set k whose distance d
 * satisfies |d - cutoff| <= `tol` (Angstrom, > 0) for the set's hard cutoff at step s -- the pairs at which two runs that differ by rounding (another
 * DBFR_GEMM mode, another batch of the reference) may build different graphs.  Candidates: set 0 every ligand pair, BONDED PAIRS INCLUDED (the
 * reference's ligand set is the bond edges concatenated with a radius graph over all pairs, so a bonded pair across 5 A changes the edge count
 * too); set 1 every pocket pair; sets 2 and 3 (the same pairs) ligand x pocket atoms other than CA / CB (edges at any distance), in units of the
 * graph's dynamic cutoff 0.2 tr_sigma + 5; sets 4 and 5 the bond mid-point x every atom of the graph.  The neighbour caps are ignored: pairs past
 * a cap count too, so the log may over-flag there but never under-flag.  A zero row means the step's graph is decided by margins above tol;
 * tests/test_examples.py reads it next to the edge counts.  Diagnostic: its kernel is launched only while a log is attached.  Same layout,
 * capacity rule and switch-off (log == NULL) as dbfr_model_set_edge_log.                                                                    */
int dbfr_model_set_tie_log(dbfr_model* m, int32_t* log_dev, int32_t n_steps_cap, int32_t n_graphs_cap, float tol);

/* ---- pose initialisation, on the device.
 * Replaces the per-pose real-time transforms LigInit + SCProtInit +
 * Atom14ToAllAtomsRepr (druglib/datasets/Docking/struct_init.py:16-53,114-138;
 * formatting.py:41-51) for every graph of an assembled batch at once:
 *   lig_pos       <- torsion kicks in bond order, (x - centroid) R^T + tr
 *   torsion_angle <- chi_k = sc_u * sc_torsion_edge_mask (psi kept)
 *   rec_pos       <- side chains rebuilt from the templates, compacted
 * The random draws come from the caller as a device tape in the reference's
 * draw order per pose.  b->lig_pos must hold the ligands' input conformers.     */
typedef struct {
  const float* tor_u;  /* [NTOR]  U(-pi,pi) torsion kicks                       */
  const float* rot;    /* [G,3,3] uniformly random rotation matrices, row-major  */
  const float* tr;     /* [G,3]   N(0, tr_sigma_max) translations                */
  const float* sc_u;   /* [NR,4]  U(-pi,pi) chi draws (unmasked)                 */
} dbfr_init_tape;

int dbfr_init_poses(const dbfr_model* m, const dbfr_batch* b, const dbfr_init_tape* tape, float* atom14_out,
                    void* hip_stream);

/* ---- pocket templates, on the device.
 * Replaces extract_chi_and_template (druglib/utils/obj/prot_math.py:116-241,
 * called once per pocket from SCPocketFinderDefault, pocket_pipeline.py:174-189):
 * from residue types and atom14 coordinates (unused slots zero) to the backbone
 * frames, psi/chi1..4 (radians), the per-residue default frames [n,8,4,4] and the
 * atoms' positions inside their rigid groups [n,14,3] -- the inverse of the
 * side-chain rebuild inside dbfr_sample.  All pointers are device pointers; the
 * residue tables are compiled in.  aatype in [0, 20].                            */
int dbfr_extract_templates(int32_t n_res, const int32_t* aatype, const float* atom14_pos, float* backbone_transl,
                           float* backbone_rots, float* default_frame, float* rigid_group_positions,
                           float* torsion_angle, void* hip_stream);

/* Binding-site residues of n_prot proteins in one pass (ahead of row f2): what
 * Protein.query_region / select_bs computes (druglib/utils/obj/protein.py:154-240,
 * druglib/utils/bio_utils/select_pocket.py:12-99; SCPocketFinderDefault uses mode
 * 'any', cutoff 12, all ligand atoms, pocket_pipeline.py:147-161).  Residue r of
 * protein p (rows res_ptr[p]..res_ptr[p+1]) is selected iff the squared distance
 * between one of its present atoms and one of the protein's reference points
 * (rows ref_ptr[p]..ref_ptr[p+1] of ref_pos) is <= cutoff^2; the nearest residue is
 * always selected; max_neighbors > 0 keeps only that many nearest selected
 * residues.  atoms_per_res = 37 / 14 (mode 'any'), a column subset (atom modes) or
 * 1 (centroids).  All pointers are device pointers; min_dist2 [n_res_total] and
 * res_mask [n_res_total] (0/1 bytes) are outputs.                                   */
int dbfr_select_pocket(int32_t n_prot, int32_t n_res_total, const int32_t* res_ptr, int32_t atoms_per_res,
                       const float* atom_pos, const float* atom_mask, const int32_t* ref_ptr, const float* ref_pos,
                       double cutoff, int32_t max_neighbors, float* min_dist2, uint8_t* res_mask, void* hip_stream);

/* ---- output side: what `complex_modeling`
 * (DiffBindFR/evaluation/export.py:106-312) does with the trajectories dbfr_sample
 * returns -- the per-pose metrics and the PDB text of every pose.                  */

/* Per-(pose, frame) metrics over the trajectories of ONE complex, computed where the
 * trajectories already are (device pointers, fp32):
 *   centroid  |mean(lig + c) - mean(lig_target)|          metrics/centroid.py:6-14
 *   sc_rmsd   side-chain RMSD, best of the two namings of the pi-symmetric groups,
 *             mean over residues with a side chain        metrics/scrmsd.py:64-89
 *   delta_chi |chi_pred - chi_target| per residue and chi (radians, wrapped as the
 *             reference wraps it, best of the pi-periodic alternatives, 0 where the
 *             chi does not exist)                         metrics/angbin.py:11-103
 *   chi_rate  fraction of existing chi_k with delta below chi_bound (15 degrees in
 *             the reference)                              evaluation/export.py:176-181
 *   lig_rmsd  heavy-atom RMSD, minimum over the automorphisms `perms` of the ligand
 *             graph                                       metrics/lrmsd.py:311-335
 * center[3] (host) is the pocket centre the sampler's coordinates are relative to
 * (add_center_pos, common/inference_dataset.py:57-63): it is added to both
 * trajectories and to atom14_target for sc_rmsd; lig_target is absolute.           */
typedef struct {
  int32_t n_pose, n_frame, n_lig, n_res;
  const float*   lig_traj;            /* [n_pose, n_frame, n_lig, 3]                   */
  const float*   prot_traj;           /* [n_pose, n_frame, n_res, 14, 3]               */
  const float*   lig_target;          /* [n_lig, 3]                                    */
  const float*   atom14_target;       /* [n_res, 14, 3] pocket-centred like prot_traj  */
  const float*   atom14_target_mask;  /* [n_res, 14] 0/1                               */
  const int32_t* aatype;              /* [n_res] in [0, 20]                            */
  int32_t        n_perm;              /* automorphisms (>= 1 when lig_rmsd is asked)   */
  const int32_t* perms;               /* [n_perm, n_lig]: atom perms[p][a] of the pose is compared with target atom a */
  const int32_t* heavy_mask;          /* [n_lig] 0/1 (atoms that count), or NULL = all */
  float          center[3];
  float          chi_bound;           /* radians                                       */
} dbfr_pose_metrics_in;

typedef struct {                      /* any pointer may be NULL = not wanted          */
  float* centroid;                    /* [n_pose, n_frame]                             */
  float* sc_rmsd;                     /* [n_pose, n_frame]                             */
  float* chi_rate;                    /* [n_pose, n_frame, 4]                          */
  float* delta_chi;                   /* [n_pose, n_frame, n_res, 4]                   */
  float* lig_rmsd;                    /* [n_pose, n_frame]                             */
} dbfr_pose_metrics_out;

int dbfr_pose_metrics(const dbfr_pose_metrics_in* in, const dbfr_pose_metrics_out* out, void* hip_stream);

/* PDB text of a protein (host code, all pointers host): byte-for-byte what
 * Protein.pos_update(pos14).to_pdb() writes (druglib/utils/obj/protein.py:478-537,
 * 678-800).  The static part of a structure is the topology; a pose replaces the
 * atom14 coordinates of `rows` (the pocket residues inside the protein,
 * evaluation/export.py:261-268).                                                  */
typedef struct {
  int32_t        n_res;
  const int32_t* aatype;              /* [n_res] in [0, 20] (20 = 'UNK')               */
  const float*   atom37_pos;          /* [n_res, 37, 3] coordinates of the input structure */
  const float*   atom37_mask;         /* [n_res, 37] atoms present (>= 0.5)            */
  const int32_t* residue_index;       /* [n_res] PDB residue numbers                   */
  const int32_t* chain_index;         /* [n_res] 0-based chain ids (A..Z, AA, BA, ...) */
  const double*  b_factors;           /* [n_res, 37]                                   */
  const char*    remark;              /* first line, or NULL for none                  */
} dbfr_pdb_topology;

/* Formats one structure into out (capacity cap bytes, no terminating NUL needed) and
 * returns the byte count; if cap is too small nothing is written and the required
 * count is returned.  n_rows == 0: the topology's own coordinates.  rows == NULL
 * with n_rows == n_res: pos14 covers every residue in order.  model < 0: no ENDMDL. */
int64_t dbfr_pdb_format(const dbfr_pdb_topology* topo, int32_t n_rows, const int32_t* rows, const float* pos14,
                        int32_t model, int32_t add_end, char* out, int64_t cap);

/* Writes n_pose files: paths[i] receives the structure with pos14[i] ([n_pose, n_rows,
 * 14, 3]) on n_threads host threads (<= 0: one per pose up to the core count).      */
int dbfr_pdb_write_files(const dbfr_pdb_topology* topo, int32_t n_rows, const int32_t* rows, const float* pos14,
                         int32_t n_pose, const char* const* paths, int32_t n_threads);

/* (ABI 6) The ATOM records of dbfr_pdb_format(topo, n_rows, rows, ...) as coordinate sources, in record order (the same walk
 * as the text writer, so an XTC frame built from the map lists the atoms of the PDB in its order).  code[k] of record k:
 * DBFR_XTC_POCKET(j, s) = atom14 slot s of pos14 row j (the row of rows[] the residue is in), or DBFR_XTC_STATIC(m) = the
 * coordinate the writer prints for a residue no row covers, written to static_pos[m] ([n_static, 3], m counts up from 0).
 * Returns the number of ATOM records (nothing is written when it exceeds cap); *n_static (may be NULL) the static ones. */
int64_t dbfr_pdb_atom_map(const dbfr_pdb_topology* topo, int32_t n_rows, const int32_t* rows, int32_t* code, float* static_pos,
                          int64_t cap, int64_t* n_static);

/* (ABI 6) A ligand's PDB block (what Chem.MolToPDBBlock gives for a hydrogen-free mol without residue info: COMPND, HETATM
 * ... 'UNL', CONECT, END) prepared once as text; per pose only columns 31-54 of the HETATM records change (three %8.3f).
 * Byte parity with RDKit is NOT pinned (RDKit is absent offline); the XTC bytes do not depend on this text.            */
typedef struct {
  int32_t            n_atoms;
  const char*        head;       /* lines before the atom records (COMPND), each newline-terminated, may be ""        */
  const char* const* atom_line;  /* [n_atoms] HETATM records without newline, >= 54 chars; columns 31-54 are replaced   */
  const char*        tail;       /* CONECT records and END, each newline-terminated                                   */
} dbfr_pdb_ligand;

/* PLComplex(protein, ligand).to_pdb() (druglib/utils/obj/complex.py:165-191): the protein's REMARK lines, the ligand's lines
 * up to its first CONECT, the protein's other lines, the ligand's remaining lines and a final newline, joined by newlines.
 * Protein text as dbfr_pdb_format(topo, n_rows, rows, pos14, -1, 1); lig_pos [n_atoms, 3].  Returns the byte count (nothing
 * written when it exceeds cap).                                                                                         */
int64_t dbfr_complex_pdb_format(const dbfr_pdb_topology* topo, int32_t n_rows, const int32_t* rows, const float* pos14,
                                const dbfr_pdb_ligand* lig, const float* lig_pos, char* out, int64_t cap);
/* paths[i] receives the complex of pos14[i] ([n_file, n_rows, 14, 3]) and lig_pos[i] ([n_file, n_atoms, 3]) on n_threads host
 * threads (<= 0: OMP_NUM_THREADS when set, else 16; never more than n_file).                                             */
int dbfr_complex_pdb_write_files(const dbfr_pdb_topology* topo, int32_t n_rows, const int32_t* rows, const float* pos14,
                                 const dbfr_pdb_ligand* lig, const float* lig_pos, int32_t n_file, const char* const* paths,
                                 int32_t n_threads);

/* SD file of a ligand pose (host code, all pointers host): what the reference writes per pose as `lig_final.sdf`
 * (DiffBindFR/evaluation/export.py:97-103,236-244: Ligand3D.pos_update(pose) -> Chem.SDWriter).  The V2000 mol block of
 * the (hydrogen-free) ligand is prepared once as text; per pose only the coordinate columns change.
 * Byte parity with RDKit's SDWriter is NOT pinned (RDKit is absent offline): the block follows the CTfile V2000 layout
 * RDKit reads and writes (%10.4f coordinates), header program line "DBFR-HIP".                                        */
typedef struct {
  int32_t            n_atoms;    /* atoms of the block = rows of a pose                                             */
  const char*        header;     /* 3 header lines + counts line, each newline-terminated                            */
  const char* const* atom_tail;  /* [n_atoms] atom line after the 30 coordinate columns (" C   0  0 ...", no newline) */
  const char*        trailer;    /* bond block, property block, "M  END", data items, "$$$$", newline-terminated      */
} dbfr_sdf_template;

/* Formats one pose (pos [n_atoms,3]) into out (capacity cap) and returns the byte count; too small a cap writes nothing. */
int64_t dbfr_sdf_format(const dbfr_sdf_template* t, const float* pos, char* out, int64_t cap);
/* paths[i] receives pose i of pos [n_pose, n_atoms, 3] on n_threads host threads (<= 0: one per pose up to the cores). */
int dbfr_sdf_write_files(const dbfr_sdf_template* t, const float* pos, int32_t n_pose, const char* const* paths,
                         int32_t n_threads);

/* ---- MDN pose scorer: the network forward of the KarmaDock scorer the reference runs on the
 * sampled poses (DiffBindFR/scoring/architecture/KarmaDock_sc.py:58-101, called from DiffBindFR/common/engines.py:230-302):
 * graph-transformer ligand encoder, GVP pocket encoder, mixture-density head, score = sum over (ligand atom, residue)
 * pairs within 5 A of the 10-component mixture density at their distance.  Inputs are the featurised tensors the
 * reference's HeteroData batch holds (the RDKit / openfold featurisation stays on the host, outside this path).       */
typedef struct dbfr_mdn_model dbfr_mdn_model;
/* tensors: the reference module's state_dict entries (names relative to KarmaDock: "lig_encoder...", "pro_encoder...",
 * "mdn_layer..."); tensors of modules the scoring forward never calls (egnn_layers, gates, ...) may be present.        */
int  dbfr_mdn_model_create(const dbfr_tensor* tensors, int32_t n_tensors, dbfr_mdn_model** out);
void dbfr_mdn_model_destroy(dbfr_mdn_model* m);

typedef struct {                      /* device pointers; graphs are contiguous node ranges                              */
  int32_t B, NL, EL, NR, EP;          /* graphs, ligand atoms, directed covalent ligand edges, residues, pocket edges     */
  const int32_t* lig_ptr;             /* [B+1]                                                                            */
  const float*   lig_node_s;          /* [NL,89]   data['ligand'].node_s                                                  */
  const float*   lig_edge_s;          /* [EL,20]   edge_s[cov_edge_mask]                                                  */
  const int32_t* lig_edge_src;        /* [EL]      edge_index[0] (row)                                                    */
  const int32_t* lig_edge_dst;        /* [EL]      edge_index[1] (col): attention is normalised over the edges into col   */
  const int32_t* lig_in_ptr;          /* [NL+1]    CSR over lig_in_edge by col                                            */
  const int32_t* lig_in_edge;         /* [EL]      edge ids grouped by col, ascending inside a group                      */
  const float*   lig_pos;             /* [NL,3]    data['ligand'].xyz (the pose)                                          */
  const float*   lig_s_in;            /* [NL,128]  optional: ligand embeddings computed before (they do not depend on the
                                                   pose), NULL = run the ligand encoder                                   */
  const int32_t* res_ptr;             /* [B+1]                                                                            */
  const float*   pro_node_s;          /* [NR,9]                                                                           */
  const float*   pro_node_v;          /* [NR,3,3]                                                                         */
  const int32_t* pro_edge_src;        /* [EP]      edge_index[0] (message source j)                                       */
  const int32_t* pro_edge_dst;        /* [EP]      edge_index[1] (target i); edges GROUPED BY TARGET (knn_graph order)    */
  const int32_t* pro_in_ptr;          /* [NR+1]    CSR over the edge array by target                                      */
  const float*   pro_edge_s;          /* [EP,21]                                                                          */
  const float*   pro_edge_v;          /* [EP,1,3]                                                                         */
  const int32_t* pro_seq;             /* [NR]      residue type ids (< 31)                                                */
  const float*   pro_xyz_full;        /* [NR,14,3] atom14 coordinates of the pose (unused slots as the featuriser leaves them) */
  float          dist_threshold;      /* pairs farther apart contribute 0 (KarmaDock.forward passes 5.0); <= 0 = 5.0       */
} dbfr_mdn_batch;

int dbfr_mdn_workspace_bytes(const dbfr_mdn_batch* b, size_t* bytes);
/* score [B]; lig_s_out [NL,128] / pro_s_out [NR,128] optional (embeddings, e.g. to reuse lig_s for the other poses).      */
int dbfr_mdn_forward(dbfr_mdn_model* m, const dbfr_mdn_batch* b, float* score, float* lig_s_out, float* pro_s_out,
                     void* workspace, size_t workspace_bytes, void* hip_stream);

/* The pocket half of the scorer's input on the device, for n_graph pockets / poses at once: what `get_protein_feature`
 * (DiffBindFR/scoring/dataset/protein_feature.py:137-216) computes behind its PDB parser from residue types (< 20) and
 * atom14 coordinates with absent atoms at the origin (= dbfr_sample's atom14 output + the pocket centre): node_s [n_res,9],
 * node_v [n_res,3,3], the topk (<= 32; the reference uses 30) nearest CA neighbours of every residue as edges j -> i grouped
 * by i (edge_src / edge_dst / in_ptr [n_res+1]), edge_s [E,21], edge_v [E,3].  edge_ptr [n_graph+1]: first edge of every
 * pocket, E_g = n_g * min(topk, n_g - 1) (the caller knows the residue counts).  Pockets of at most 1024 residues.        */
int dbfr_mdn_pocket_features(int32_t n_graph, int32_t n_res, const int32_t* res_ptr, const int32_t* edge_ptr,
                             const int32_t* aatype, const float* atom14_pos, int32_t topk, float* node_s, float* node_v,
                             int32_t* edge_src, int32_t* edge_dst, int32_t* in_ptr, float* edge_s, float* edge_v,
                             void* hip_stream);

/* ---- Vina-function refinement of sampled poses (the error-correction stage the reference delegates to `smina --minimize`,
 * DiffBindFR/app/predict.py:156-191; built here as a specified refinement, numeric parity with smina is not pinned).
 * The AutoDock Vina scoring function (Trott & Olson, J. Comput. Chem. 2010) on a rigid receptor, heavy atoms only, XS atom
 * types 0..15 = C_H C_P N_P N_D N_A N_DA O_P O_D O_A O_DA S_P P_P F_H Cl_H Br_H I_H and 17 = Met_D (a metal ion: radius 1.2 A,
 * donor, neither hydrophobic nor acceptor), 16 and any other value = DUMMY (takes part in no term).  Pairs with r < 8 A, d = r - R_i - R_j:  gauss1 exp(-(d/0.5)^2) x -0.035579, gauss2 exp(-((d-3)/2)^2) x -0.005156,
 * repulsion d^2 (d < 0) x 0.840245, hydrophobic (both hydrophobic: 1 below 0.5, linear to 0 at 1.5) x -0.035069, hbond (donor
 * with acceptor, either way: 1 below -0.7, linear to 0 at 0) x -0.587439.  E_inter over (ligand, receptor) pairs, E_intra
 * over the listed ligand pairs; objective = E_inter + E_intra; affinity = E_inter / (1 + 0.05846 N_rot), N_rot = the graph's
 * torsions (tor_ptr).  diffbindfr_amd/vina.py types the atoms and builds the pair lists; docs/vina.md states it all.
 * Receptor atoms of a pose = its pocket atoms in `batch` (rec_pos, rec_type) + optional extra atoms (ext_*).           */
typedef struct {
  const dbfr_batch* batch;   /* host struct of device pointers: lig_ptr, lig_pos, bond_src/dst, tor_ptr, tor_bond, rot_mask(_off), atm_ptr, rec_pos */
  const int8_t*  lig_type;   /* [NL] XS type of every ligand atom                                                       */
  const int8_t*  rec_type;   /* [NA] XS type of every pocket atom                                                       */
  const int32_t* pair_ptr;   /* [G+1] CSR of the intra-ligand pairs by graph                                           */
  const int32_t* pair_ij;    /* [n_pairs, 2] global ligand atom indices, each unordered pair once                       */
  int32_t        n_pairs;
  const int32_t* ext_ptr;    /* [G+1] extra receptor atoms per graph, or NULL = none                                    */
  const float*   ext_pos;    /* [n_ext, 3] in the frame of lig_pos                                                      */
  const int8_t*  ext_type;   /* [n_ext]                                                                                 */
  int32_t        max_tor;    /* host-known maxima over the graphs: torsions (<= 58), extra atoms                         */
  int32_t        max_ext;
} dbfr_vina_in;

typedef struct {
  int32_t max_iters;         /* BFGS iterations (accepted steps), default 100                                           */
  float   grad_tol;          /* stop once max |dE/dq| < grad_tol, default 1e-3                                          */
  float   margin;            /* receptor candidates within 8 A + margin; collected again after a move of margin / 2 (2)  */
} dbfr_vina_opts;

/* Device workspace (receptor candidate lists): G x (max_na + max_ext) x 16 bytes.  Refuses (DBFR_ERR_ARG) ligands of more than
 * 256 atoms or 58 torsions (the minimiser's (6 + n_tor)^2 inverse Hessian is held in LDS) and pockets of more than 8192 atoms.  A
 * graph whose counts exceed the stated maxima, or whose torsion bond lies outside its atoms, gets NaN terms and iters = -1 and
 * is not touched.                                                                                         */
int dbfr_vina_workspace_bytes(const dbfr_vina_in* in, size_t* bytes);
/* At the poses in batch->lig_pos: terms [G,8] = {gauss1, gauss2, repulsion, hydrophobic, hbond (weighted inter terms), E_intra,
 * objective, affinity}; grad_rigid [G,6] = {sum_i dE/dx_i, sum_i (x_i - c) x dE/dx_i} (c = ligand centroid); grad_tor [NTOR]:
 * sum over the rot_node_mask row of (a x (x_i - x_v)) . dE/dx_i, a = unit (x_u - x_v), (u, v) = (bond_src, bond_dst) of the
 * torsion's bond -- the sign conventions of the sampler's ligand update.  Any output may be NULL.  One workgroup per pose.    */
int dbfr_vina_score(const dbfr_vina_in* in, float* terms, float* grad_rigid, float* grad_tor, void* workspace,
                    size_t workspace_bytes, void* hip_stream);
/* The same at the pose the minimiser builds from the variables q: q_rigid [G,6] = (translation, rotation vector), q_tor [NTOR]
 * torsion angles (radians), either may be NULL = 0; the positions are rebuilt from batch->lig_pos as in dbfr_vina_minimize and
 * written to lig_pos_out [NL,3] (may be NULL); grad_rigid / grad_tor receive dE/dq -- the gradient the minimiser follows (at
 * q = 0 it is the generalised gradient above).                                                                              */
int dbfr_vina_score_at(const dbfr_vina_in* in, const float* q_rigid, const float* q_tor, float* lig_pos_out, float* terms,
                       float* grad_rigid, float* grad_tor, void* workspace, size_t workspace_bytes, void* hip_stream);
/* BFGS over q = (translation, rotation vector, torsions) with a backtracking (Armijo) line search whose first trial moves no
 * variable by more than 0.3 (A or rad: a local search); positions are rebuilt from
 * batch->lig_pos for every trial q: torsions in tor_bond order about the current bond axis (pivot x_v), then the rotation
 * about the centroid, then the translation.  lig_pos_out [NL,3] (may be NULL; equal to batch->lig_pos = in place) receives
 * the final poses, terms [G,8] their terms as above, iters [G] the accepted steps.  A pose stops at max |dE/dq| < grad_tol,
 * after max_iters steps, or when not even a steepest-descent step lowers the objective any more.  opts NULL = defaults.     */
int dbfr_vina_minimize(const dbfr_vina_in* in, const dbfr_vina_opts* opts, float* lig_pos_out, float* terms, int32_t* iters,
                       void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- Monte-Carlo search (docs/vina.md, "Monte-Carlo search"): Vina's iterated local search around dbfr_vina_minimize, on a rigid
 * receptor.  One workgroup per (pose, chain).  A chain minimises its start (the input pose; with random_start and chain >= 1 a random
 * placement in the box), then repeats n_steps times: mutate one entity of the current pose (translation, rotation or one torsion),
 * minimise the candidate for at most step_iters BFGS steps from H = I, accept it by the Metropolis rule at `temperature` if every atom
 * lies in the box (the input pose's bounding box grown by autobox_add on every side); the lowest accepted candidate is the best,
 * and a best that came from a step is minimised once more with opts->max_iters (kept if it is not higher and still in the box).  Random numbers: Philox4x32-10, key = seed, counter =
 * (stream low, stream high, chain, slot): a (pose, chain) result depends on its inputs, the seed, its stream and its chain only.   */
typedef struct {
  int32_t  chains;           /* chains per pose (smina's exhaustiveness), default 8; >= 1                                       */
  int32_t  n_steps;          /* Monte-Carlo steps per chain, default 64; >= 0 (0 = dbfr_vina_minimize per chain)                */
  int32_t  step_iters;       /* BFGS steps per candidate; < 0 = (25 + n_atoms) / 3 (Vina's), 0 = evaluate the mutated pose only */
  float    temperature;      /* kcal/mol, default 1.2; > 0                                                                      */
  float    amplitude;        /* A: radius of the translation ball; the rotation ball is amplitude / r_g rad; default 2         */
  float    autobox_add;      /* A added to the input pose's bounding box on every side, default 4                               */
  int32_t  random_start;     /* != 0: chains >= 1 start from a random placement; chain 0 always starts from the input pose      */
  uint64_t seed;             /* the Philox key                                                                                  */
} dbfr_vina_search_opts;

/* Device workspace of dbfr_vina_search: chains x the workspace of dbfr_vina_workspace_bytes.  The checks of that call apply.     */
int dbfr_vina_search_workspace_bytes(const dbfr_vina_in* in, int32_t chains, size_t* bytes);
/* opts NULL = the defaults of dbfr_vina_minimize, search_opts NULL = the defaults above.  stream [G] int64 (device): the Philox
 * stream of every pose.  best_pos [chains, NL, 3]: each chain's best pose; cur_pos [chains, NL, 3] (may be NULL): each chain's
 * current pose after the last step; terms [chains, G, 8]: the terms of best_pos as dbfr_vina_score gives them; iters [chains, G]:
 * BFGS steps over all minimisations of the chain; accepted [chains, G]: accepted Monte-Carlo steps; log (may be NULL)
 * [chains, G, n_steps, 8] floats per step: {entity (0 translation, 1 rotation, 2 + k torsion k), E_c (the candidate's objective),
 * in_box, the Metropolis u, accepted, E_cur after the step, E_best after the step, BFGS steps of the candidate}.  Energies are
 * compared as the floats the log holds.  A graph dbfr_vina_minimize refuses gets NaN terms, iters = -1 and accepted = 0 in every
 * chain and is not touched.  chains < 1, n_steps < 0 or temperature <= 0 (or not a number): DBFR_ERR_ARG.                         */
int dbfr_vina_search(const dbfr_vina_in* in, const dbfr_vina_opts* opts, const dbfr_vina_search_opts* search_opts, const int64_t* stream,
                     float* best_pos, float* cur_pos, float* terms, int32_t* iters, int32_t* accepted, float* log, void* workspace,
                     size_t workspace_bytes, void* hip_stream);
/* Host test hooks of the search's random numbers (no device needed).  dbfr_test_philox4x32: one Philox4x32-10 block.
 * dbfr_test_vina_mutation: the mutation of Monte-Carlo step `step` (1-based) of (seed, stream, chain) for a ligand of n_tor
 * torsions: *entity and q [6 + n_tor] (translation, rotation vector, torsions; all but the chosen entity's entries 0).          */
int dbfr_test_philox4x32(const uint32_t* ctr, const uint32_t* key, uint32_t* out);
int dbfr_test_vina_mutation(uint64_t seed, int64_t stream, int32_t chain, int32_t step, int32_t n_tor, float amplitude, float r_g,
                            int32_t* entity, float* q);

/* ---- The same refinement with flexible pocket side chains (docs/vina.md, "Flexible side chains"; the same kernel code in a
 * second instantiation).  Receptor atoms of a pose are numbered pocket atoms first (0 .. na_g - 1: rec_pos under atm_ptr), then
 * the graph's extra atoms (na_g ..).  Each graph lists some pocket atoms as flexible and an ordered list of flexible torsions:
 * torsion k has the axis (b, c) (two pocket atoms, pivot b, direction b -> c) and turns the listed flexible atoms; torsions are
 * applied in list order about the current axis, as the ligand's are; the ligand's rigid motion and centroid involve ligand atoms
 * only.  objective = E_inter + E_intra + E_rec: E_inter over (ligand, receptor) pairs, fixed and flexible receptor atoms alike;
 * E_rec = the same five weighted terms over (flexible, fixed) and (flexible, flexible) pairs except the partners on the flexible
 * atom's exclusion list (the receptor atoms within 3 bonds).  affinity = E_inter / (1 + 0.05846 N_rot), N_rot = ligand torsions.
 * Variables q = (translation, rotation vector, ligand torsions, flexible torsions); BFGS, line search and stop rules as above.
 * Limits (DBFR_ERR_ARG): max_nl + max_flex + max_anchor <= 256 (an anchor = an axis end that is not flexible, one per end),
 * 6 + max_tor + max_ftor <= 128 variables, exclusion lists of at most 32 atoms, max_na <= 8192.  A graph that exceeds the stated
 * maxima or whose lists are inconsistent gets NaN terms and iters = -1 and is not touched.                                     */
typedef struct {
  const dbfr_vina_in* base;
  const int32_t* flex_ptr;    /* [G+1] flexible atoms by graph                                                           */
  const int32_t* flex_atom;   /* [n_flex] graph-local pocket atom index, ascending within a graph                        */
  const int32_t* ftor_ptr;    /* [G+1] flexible torsions by graph                                                        */
  const int32_t* ftor_bc;     /* [n_ftor, 2] axis (b, c), graph-local pocket atom indices                                */
  const int32_t* turn_ptr;    /* [n_ftor+1] CSR over the torsions of all graphs into turn                                */
  const int32_t* turn;        /* the atoms a torsion turns, as positions in its graph's flexible atom list               */
  const int32_t* excl_ptr;    /* [n_flex+1] CSR over the flexible atoms of all graphs into excl                          */
  const int32_t* excl;        /* receptor atom indices of the graph, at most 32 per list                                 */
  int32_t        n_flex;      /* flex_ptr[G]                                                                             */
  int32_t        n_ftor;      /* ftor_ptr[G]                                                                             */
  int32_t        max_flex;    /* host-known maxima over the graphs: flexible atoms, flexible torsions, axis anchors,     */
  int32_t        max_ftor;    /* exclusion list length                                                                   */
  int32_t        max_anchor;
  int32_t        max_excl;
  const void*    host;        /* NULL, or a dbfr_vina_flex_in whose eight array pointers are HOST copies of the same arrays
                                 (base is not read): every list is then validated before the launch (DBFR_ERR_ARG): CSR shapes,
                                 per-graph counts against the maxima, indices against max_na (+ max_ext for excl)            */
} dbfr_vina_flex_in;

/* The workspace of dbfr_vina_workspace_bytes(in->base); runs every check of the flexible calls.                           */
int dbfr_vina_flex_workspace_bytes(const dbfr_vina_flex_in* in, size_t* bytes);
/* dbfr_vina_score_at with q_flex [n_ftor] (NULL = 0): rec_pos_out [NA,3] receives the pocket atoms (fixed atoms copied bit for
 * bit), terms [G,10] = the eight of dbfr_vina_score (objective including E_rec), E_rec, E_rec of the first evaluation;
 * grad_flex [n_ftor] = dE/dq_flex.  Any output may be NULL.                                                                */
int dbfr_vina_flex_score_at(const dbfr_vina_flex_in* in, const float* q_rigid, const float* q_tor, const float* q_flex,
                            float* lig_pos_out, float* rec_pos_out, float* terms, float* grad_rigid, float* grad_tor,
                            float* grad_flex, void* workspace, size_t workspace_bytes, void* hip_stream);
/* dbfr_vina_minimize over the larger q: q_flex_out [n_ftor] receives the final flexible torsion angles (radians), terms[9] the
 * E_rec of the starting pose.  With no flexible atoms in any graph the results equal dbfr_vina_minimize's bit for bit.       */
int dbfr_vina_flex_minimize(const dbfr_vina_flex_in* in, const dbfr_vina_opts* opts, float* lig_pos_out, float* rec_pos_out,
                            float* q_flex_out, float* terms, int32_t* iters, void* workspace, size_t workspace_bytes,
                            void* hip_stream);

/* ---- The Monte-Carlo search with flexible pocket side chains (docs/vina.md, "Search with flexible side chains"): the rule of
 * dbfr_vina_search over the variables of dbfr_vina_flex_minimize, in a second instantiation of the same kernel.  A step draws its
 * entity among 2 + ligand torsions + flexible torsions (dbfr_test_vina_mutation with n_tor = their sum): entity 2 + ntl + k sets
 * flexible torsion k of the graph to a uniform angle in [-pi, pi).  The Metropolis energy is the flexible objective
 * E_inter + E_intra + E_rec; the box test reads the ligand's atoms only; step_iters < 0 = (25 + ligand atoms + flexible atoms) / 3;
 * with random_start the chains >= 1 re-place the ligand only (the draws of dbfr_vina_search) and keep the input side chains.
 * With no flexible atom in any graph the results equal dbfr_vina_search's bit for bit.                                          */
/* Device workspace of dbfr_vina_flex_search: chains x the workspace of dbfr_vina_flex_workspace_bytes; every check of the flexible
 * calls runs.                                                                                                                */
int dbfr_vina_flex_search_workspace_bytes(const dbfr_vina_flex_in* in, int32_t chains, size_t* bytes);
/* opts, search_opts, stream, iters, accepted and log [chains, G, n_steps, 8] as in dbfr_vina_search.  best_pos [chains, NL, 3] and
 * best_rec [chains, NA, 3]: each chain's best ligand pose and its pocket atoms (fixed atoms copied bit for bit); q_flex_out
 * [chains, n_ftor]: the best pose's flexible torsion angles against the input, in [-pi, pi) (required when n_ftor > 0); cur_pos /
 * cur_rec (either may be NULL): each chain's current pose after the last step; terms [chains, G, 10] as dbfr_vina_flex_score_at
 * gives them for the best pose, terms[9] = E_rec at the first evaluation of the chain's start minimisation.  The refusals of
 * dbfr_vina_search and of dbfr_vina_flex_minimize both apply before any launch (DBFR_ERR_ARG), the validation of the lists through
 * `host` included.  A graph dbfr_vina_flex_minimize refuses gets NaN terms, iters = -1 and accepted = 0 in every chain and is not
 * touched.                                                                                                                   */
int dbfr_vina_flex_search(const dbfr_vina_flex_in* in, const dbfr_vina_opts* opts, const dbfr_vina_search_opts* search_opts,
                          const int64_t* stream, float* best_pos, float* best_rec, float* q_flex_out, float* cur_pos, float* cur_rec,
                          float* terms, int32_t* iters, int32_t* accepted, float* log, void* workspace, size_t workspace_bytes,
                          void* hip_stream);

/* ---- Distinct binding modes of sampled poses (csrc/modes.hip; docs/modes.md).  A batch of G groups (one group = the poses
 * of one ligand in one pocket frame), group g holding P_g poses of N_g atoms and n_perm_g automorphisms (identity included):
 *   R_g[i, j] = min over sigma of sqrt( (1/|H|) sum_{a in H} |x_i[sigma(a)] - x_j[a]|^2 )
 * without superposition (the pocket frame fixes the pose): the lig_rmsd of dbfr_pose_metrics with pose i as the pose and
 * pose j as the target.  H = the heavy atoms (heavy_mask, NULL = all atoms).  Only i < j is computed; R_g[j, i] holds the same
 * bits and the diagonal an exact 0.  Every (pose pair, automorphism) sum runs serially over the atoms in index order, so a
 * group's matrix is bitwise the same alone or in any batch, whatever the path and tiling.  Groups of at most 4096 poses
 * and 1024 atoms.                                                                                                           */
typedef struct {
  int32_t        n_group;
  const int32_t* pose_ptr;   /* [G+1] first pose of every group (P_g = pose_ptr[g+1] - pose_ptr[g])                       */
  const int32_t* atom_ptr;   /* [G+1] first atom of every group (N_g); heavy_mask is indexed by atom_ptr[g] + a           */
  const int32_t* perm_ptr;   /* [G+1] first automorphism of every group (n_perm_g >= 1)                                   */
  const float*   pos;        /* group by group [P_g, N_g, 3]: group g starts at float 3 * sum_{h<g} P_h N_h              */
  const int32_t* perms;      /* group by group [n_perm_g, N_g]: group g starts at sum_{h<g} n_perm_h N_h; atom perms[p][a]
                                of pose i is compared with atom a of pose j (the convention of dbfr_pose_metrics_in)       */
  const int32_t* heavy_mask; /* [atom_ptr[G]] 0/1, or NULL = every atom counts                                            */
  int32_t        max_pose;   /* host-known maxima over the groups (<= 4096 poses, <= 1024 atoms); a group above them gets */
  int32_t        max_atom;   /*   NaN everywhere in its matrix (and -1 / 0 in the selection outputs)                     */
  int32_t        path;       /* 0 = by group (a lane per pose pair below 32 automorphisms, a wave per pair from 32 on);
                                1 / 2 = always the lane / wave path (same bits; for tests and tuning)                       */
  int32_t        tile_rows;  /* poses per LDS tile, 0 = as many as fit (same bits whatever the value; for tests)         */
} dbfr_pose_rmsd_in;

/* rmsd_out [sum_g P_g^2]: R_g row-major at out_off[g] = sum_{h<g} P_h^2.  One launch for the whole batch.                */
int dbfr_pose_rmsd_matrix(const dbfr_pose_rmsd_in* in, float* rmsd_out, void* hip_stream);

typedef struct {
  int32_t num_modes;         /* at most this many modes per group, 0 = unlimited (default 9)                              */
  int32_t higher_is_better;  /* 0: lower score is better (Vina affinity), 1: higher is better (MDN score)                  */
  float   min_rmsd;          /* a kept mode lies at least this far from every better mode, > 0 (default 1 A)             */
  float   cluster_rmsd;      /* a pose joins its nearest mode within this RMSD, >= min_rmsd (default 2 A)                 */
  float   energy_range;      /* keep only modes scoring within this of the best (lower is better only); < 0 = off        */
} dbfr_modes_opts;

/* Per group, on one workgroup: the poses ordered by score (ties by pose index, NaN scores last); a greedy walk keeps a pose
 * when its RMSD to every mode kept so far is >= min_rmsd (NaN RMSD: not kept) and its score lies within energy_range of the
 * best, and stops after num_modes modes or at the first NaN score (never kept); every pose then joins the kept mode of
 * smallest RMSD (ties: the better-ranked mode) if that RMSD is <= cluster_rmsd.  rmsd = dbfr_pose_rmsd_matrix's output
 * for the same `in` (only n_group and pose_ptr / max_pose are read), score [pose_ptr[G]].  Outputs (device): mode_rank
 * [pose_ptr[G]] = the pose's rank among the modes or -1, mode_id [pose_ptr[G]] = the rank of the mode whose cluster the
 * pose joined or -1, cluster_size [pose_ptr[G]]: entry pose_ptr[g] + r = the poses in the cluster of mode r of group g
 * (0 from the number of modes on).  Groups of at most 4096 poses (max_pose above that: DBFR_ERR_ARG).  opts NULL = defaults. */
int dbfr_select_modes(const dbfr_pose_rmsd_in* in, const float* rmsd, const float* score, const dbfr_modes_opts* opts,
                      int32_t* mode_rank, int32_t* mode_id, int32_t* cluster_size, void* hip_stream);

/* ---- PoseBusters-style physical validity checks of poses (csrc/posecheck.hip; docs/posecheck.md).  A batch of G groups (one
 * group = the frames of one ligand in one complex), group g holding F_g frames of N_g ligand heavy atoms (L), M_g pocket atoms
 * per frame and S_g static receptor atoms shared by its frames; R = pocket + static atoms.  r = van der Waals radii (given per
 * atom).  Per frame:
 *   min_dist    d_min = min over a in L, b in R of d_ab                     (protein-ligand_maximum_distance: d_min <= max_distance)
 *   min_ratio   rho = min d_ab / (r_a + r_b); n_clash = pairs with ratio < clash_ratio (minimum_distance_to_protein: rho >= clash_ratio)
 *   vol_lig, vol_overlap  on the lattice {grid * k, k in Z^3}: V_L = points p with |p - x_a| < vol_scale * r_a for some a in L,
 *               V_R the same over R; |V_L| and |V_L n V_R|           (volume_overlap_with_protein: |V_L n V_R| / |V_L| <= vol_overlap)
 *   int_min_ratio  min d / (r_a + r_b) over the listed internal pairs (+inf: none); n_int_clash = pairs below internal_ratio
 *                                                                       (internal_steric_clash: int_min_ratio >= internal_ratio)
 *   flat_dev    over the listed flatness bonds: the largest distance of a bond's atoms from their least-squares plane (0: none)
 *                                                                       (double_bond_flatness: flat_dev <= flat_tol)
 *   n_stereo_flip  stereo bonds (s_u, u, v, s_v) whose sign of cos(dihedral) differs from the given input sign
 *                                                                       (double_bond_stereochemistry: n_stereo_flip == 0)
 * Every reduction is a minimum, a maximum or an integer count, so a frame's outputs are bitwise the same alone or in any batch.
 * Limits: N_g <= 256 ligand atoms, <= 32640 internal pairs, <= 64 flatness and <= 64 stereo bonds per group (max_* above them:
 * DBFR_ERR_ARG).  Receptor atoms are not limited; the receptor atoms close enough to a ligand atom to share a lattice point with
 * it (d_ab < vol_scale (r_a + r_b) + 0.01) are compacted into LDS, at most 2048 per frame: beyond that the lattice pass of the
 * frame tests every receptor atom from memory instead (same bits, slower).                                                 */
typedef struct {
  int32_t        n_group;
  int32_t        n_frame;        /* frame_ptr[G]: one workgroup per frame                                                   */
  const int32_t* frame_ptr;      /* [G+1] first frame of every group; outputs are indexed by frame                          */
  const int32_t* lig_ptr;        /* [G+1] first atom of every group in lig_rad (N_g = lig_ptr[g+1] - lig_ptr[g], >= 1)       */
  const int64_t* lig_pos_off;    /* [G] first row of group g in lig_pos: frame k of g at rows lig_pos_off[g] + k N_g           */
  const float*   lig_pos;        /* [rows, 3]                                                                               */
  const float*   lig_rad;        /* [lig_ptr[G]] radii in (0, 4]                                                            */
  const int32_t* pocket_ptr;     /* [G+1] first pocket atom of every group in pocket_rad (M_g atoms per frame, may be 0)     */
  const int64_t* pocket_pos_off; /* [G] frame k of g at rows pocket_pos_off[g] + k M_g of pocket_pos                         */
  const float*   pocket_pos;
  const float*   pocket_rad;
  const int32_t* static_ptr;     /* [G+1] static atoms of every group in static_pos / static_rad, or NULL = none              */
  const float*   static_pos;     /* [static_ptr[G], 3] in the frame of lig_pos                                              */
  const float*   static_rad;
  const int32_t* pair_ptr;       /* [G+1] internal pairs of every group                                                     */
  const int32_t* pair_ij;        /* [pair_ptr[G], 2] local ligand atom indices                                              */
  const int32_t* flat_ptr;       /* [G+1] flatness bonds of every group                                                     */
  const int32_t* flat_atoms;     /* [flat_ptr[G], 8] local atom indices of the fitted atoms (>= 4), -1 padded               */
  const int32_t* stereo_ptr;     /* [G+1] stereo bonds of every group                                                       */
  const int32_t* stereo_atoms;   /* [stereo_ptr[G], 4] (s_u, u, v, s_v) local atom indices                                  */
  const int8_t*  stereo_sign;    /* [stereo_ptr[G]] +1 / -1: sign of cos(dihedral) in the input conformer                    */
  int32_t        max_lig;        /* host-known maxima over the groups (<= 256, 32640, 64, 64); a group above them gets NaN    */
  int32_t        max_pair;       /*   outputs, -1 counts and passed = 0                                                     */
  int32_t        max_flat;
  int32_t        max_stereo;
  int32_t        cand_cap;       /* receptor candidates kept in LDS per frame, 0 = 2048 (same bits whatever the value; tests) */
} dbfr_pose_check_in;

typedef struct {
  float clash_ratio;             /* minimum_distance_to_protein threshold, default 0.75                                     */
  float max_distance;            /* protein-ligand_maximum_distance threshold (A), default 5.0                              */
  float vol_scale;               /* sphere radius = vol_scale * r for the lattice, (0, 2], default 0.8                       */
  float vol_overlap;             /* volume_overlap_with_protein threshold, default 0.075                                    */
  float internal_ratio;          /* internal_steric_clash threshold, default 0.7                                            */
  float flat_tol;                /* double_bond_flatness threshold (A), default 0.25                                        */
  float grid;                    /* lattice spacing h (A), [0.05, 1], default 0.25                                           */
} dbfr_pose_check_opts;

typedef struct {                 /* device arrays [n_frame]; any may be NULL                                                */
  float*   min_dist;
  float*   min_ratio;
  int32_t* n_clash;
  int32_t* vol_lig;
  int32_t* vol_overlap;
  float*   int_min_ratio;
  int32_t* n_int_clash;
  float*   flat_dev;
  int32_t* n_stereo_flip;
  int32_t* passed;               /* bit k = check k passed, in the order minimum_distance_to_protein, protein-ligand_maximum_
                                    distance, volume_overlap_with_protein, internal_steric_clash, double_bond_flatness,
                                    double_bond_stereochemistry; bit 6 = all six (pb_valid)                                 */
} dbfr_pose_check_out;

/* One launch for the whole batch.  opts NULL = defaults.                                                                    */
int dbfr_pose_check(const dbfr_pose_check_in* in, const dbfr_pose_check_opts* opts, const dbfr_pose_check_out* out,
                    void* hip_stream);

/* ---- Protein-ligand interaction fingerprints of poses (csrc/interactions.hip; docs/interactions.md).  A batch of G groups (one
 * group = the frames of one ligand in one complex), group g holding F_g frames of N_g ligand heavy atoms, M_g pocket atoms per
 * frame and S_g static receptor atoms shared by its frames (receptor atom b of a frame: pocket atom b for b < M_g, static atom
 * b - M_g otherwise), LG_g ligand groups, RG_g receptor groups and n_res_g residues.  Atom types are the XS codes of the Vina calls
 * (0..16; hydrophobic C_H F_H Cl_H Br_H I_H, donors N_D N_DA O_D O_DA, acceptors N_A N_DA O_A O_DA).  A group (ligand or receptor)
 * is a ring (kind 0, its atoms in cyclic order), a cation centre (1) or an anion centre (2) of up to 6 atoms; its centre is the
 * centroid of its atoms IN THE FRAME, a ring's normal the normalised Newell sum  sum_k (p_k - c) x (p_k+1 - c)  (a ring whose
 * sum vanishes is dropped).  Per (frame, residue) one 16-bit word, bits named from the ligand's side (a ligand, b receptor atom,
 * d their distance; "angle(x-a..b)" is the angle at a between x and b, compared as a cosine; x over a's listed neighbours, y
 * over b's):
 *   0 Hydrophobic  both hydrophobic, d <= hydrophobic_dist
 *   1 HBDonor      a donor, b acceptor, d <= hbond_dist, every angle(x-a..b) >= hbond_angle, every angle(y-b..a) >= hbond_angle
 *   2 HBAcceptor   a acceptor, b donor, the same geometry
 *   3 Cationic     ligand cation centre - receptor anion centre <= ionic_dist
 *   4 Anionic      ligand anion centre - receptor cation centre <= ionic_dist
 *   5 CationPi     ligand cation centre, receptor ring: centre distance <= cation_pi_dist, offset <= cation_pi_offset (offset =
 *                  the distance of the cation's projection onto the ring plane from the ring centre)
 *   6 PiCation     ligand ring, receptor cation centre: the same
 *   7 FaceToFace   ring - ring: centres <= pi_dist, angle between the normals folded to [0, 90] <= face_angle, the smaller of
 *                  the two offsets (each centre projected onto the other ring's plane) <= pi_offset
 *   8 EdgeToFace   the same with the angle >= edge_angle
 *   9 XBDonor      a of type Cl_H / Br_H / I_H with a carbon among its listed neighbours (c = the first such), b acceptor,
 *                  d <= xbond_dist, angle(c-a..b) >= xbond_donor_angle, every angle(a..b-y) in [xbond_acceptor_min, xbond_acceptor_max]
 * counts [n_frame, 10]: the residues of the frame with bit k set.  Only integer ORs and counts leave the kernel, so a frame's
 * outputs are bitwise the same alone or in any batch.  A frame with a non-finite or out-of-range (|x| > 1e4) ligand or receptor
 * coordinate gets an all-zero row and counts of -1.  Limits: N_g <= 256, LG_g <= 32, n_res_g <= 16384 (max_* above them:
 * DBFR_ERR_ARG).  Receptor atoms and receptor groups are not limited.                                                       */
typedef struct {
  int32_t        n_group;
  int32_t        n_frame;        /* frame_ptr[G]: one workgroup per frame                                                   */
  const int32_t* frame_ptr;      /* [G+1] first frame of every group; counts are indexed by frame                           */
  const int32_t* lig_ptr;        /* [G+1] first atom of every group in lig_type / lig_nbr (N_g >= 1)                         */
  const int64_t* lig_pos_off;    /* [G] first row of group g in lig_pos: frame k of g at rows lig_pos_off[g] + k N_g           */
  const float*   lig_pos;        /* [rows, 3]                                                                               */
  const int8_t*  lig_type;       /* [lig_ptr[G]] XS codes                                                                   */
  const int32_t* lig_nbr;        /* [lig_ptr[G], 3] local indices of up to 3 bonded heavy neighbours, -1 padded              */
  const int32_t* lgrp_ptr;       /* [G+1] ligand groups of every group                                                      */
  const int32_t* lgrp;           /* [lgrp_ptr[G], 8]: kind, 6 local atom indices (-1 padded, at least 1), 0                  */
  const int32_t* pocket_ptr;     /* [G+1] first pocket atom of every group in pocket_meta (M_g atoms per frame, may be 0)    */
  const int64_t* pocket_pos_off; /* [G] frame k of g at rows pocket_pos_off[g] + k M_g of pocket_pos                         */
  const float*   pocket_pos;
  const int32_t* pocket_meta;    /* [pocket_ptr[G], 4]: type + 256 * residue (0 .. n_res_g - 1), 3 neighbours as receptor atom
                                    indices b of the group (-1 padded)                                                      */
  const int32_t* static_ptr;     /* [G+1] static atoms of every group in static_pos / static_meta, or NULL = none             */
  const float*   static_pos;     /* [static_ptr[G], 3] in the frame of lig_pos                                              */
  const int32_t* static_meta;    /* like pocket_meta                                                                        */
  const int32_t* rgrp_ptr;       /* [G+1] receptor groups of every group                                                    */
  const int32_t* rgrp;           /* [rgrp_ptr[G], 8]: kind + 256 * residue, 6 receptor atom indices b (-1 padded), 0         */
  const int32_t* res_ptr;        /* [G+1]: n_res_g = res_ptr[g+1] - res_ptr[g]                                               */
  const int64_t* bits_off;       /* [G] frame k of g writes bits[bits_off[g] + k n_res_g ...]                                */
  int32_t        max_lig;        /* host-known maxima over the groups (<= 256, 32, 16384)                                   */
  int32_t        max_lgrp;
  int32_t        max_res;
} dbfr_interactions_in;

typedef struct {                 /* lengths in A, angles in degrees; defaults in brackets                                    */
  float hydrophobic_dist;        /* [4.0]                                                                                   */
  float hbond_dist;              /* [3.5]                                                                                   */
  float hbond_angle;             /* [90]                                                                                    */
  float ionic_dist;              /* [5.5]                                                                                   */
  float cation_pi_dist;          /* [6.0]                                                                                   */
  float cation_pi_offset;        /* [2.0]                                                                                   */
  float pi_dist;                 /* [5.5]                                                                                   */
  float pi_offset;               /* [2.0]                                                                                   */
  float face_angle;              /* [30]                                                                                    */
  float edge_angle;              /* [60]                                                                                    */
  float xbond_dist;              /* [4.0]                                                                                   */
  float xbond_donor_angle;       /* [135]                                                                                   */
  float xbond_acceptor_min;      /* [90]                                                                                    */
  float xbond_acceptor_max;      /* [150]                                                                                   */
} dbfr_interactions_opts;

typedef struct {                 /* device arrays                                                                           */
  int16_t* bits;                 /* [sum_g F_g n_res_g]                                                                     */
  int32_t* counts;               /* [n_frame, 10]                                                                           */
} dbfr_interactions_out;

/* One launch for the whole batch.  opts NULL = defaults.                                                                    */
int dbfr_interactions(const dbfr_interactions_in* in, const dbfr_interactions_opts* opts, const dbfr_interactions_out* out,
                      void* hip_stream);

/* ---- Validity checks of each pose's own sampled pocket (csrc/pocketcheck.hip; docs/pocketcheck.md).  A batch of G groups (one
 * group = the frames of one complex), group g holding F_g frames of M_g pocket atoms each and S_g static receptor atoms shared by
 * its frames (receptor atom b of a frame: pocket atom b for b < M_g, static atom b - M_g otherwise), r = van der Waals radii
 * (given per atom), one residue column per atom, and a list of MOVABLE pocket atoms (side-chain atoms beyond CB), each with a
 * sorted exclusion list: the receptor atoms within 3 bonds of it.
 *   Check 1 (pocket_steric_clash).  Pair domain: unordered pairs {a, b}, a movable, b any other receptor atom not on a's
 *     exclusion list (a pair of two movable atoms is one pair).  ratio = d_ab / (r_a + r_b); a pair clashes if ratio <
 *     clash_ratio.  n_clash [n_frame, 3]: clashing pairs whose partner is movable (sc_sc), a non-movable pocket atom (sc_bb),
 *     a static atom (sc_static).  min_ratio = the minimum over the domain (+inf: empty domain), worst_pair [n_frame, 2] = the
 *     pair (a < b, receptor atom indices) of the minimum, ties to the lexicographically smallest pair, (-1, -1) for an empty
 *     domain.  res_clash (uint8 per frame and residue column) = the clashing pairs the residue takes part in (a pair inside one
 *     residue counts once), saturating at 255.  Passes if the three counts sum to <= max_clashes.
 *   Check 2 (pocket_bonds_intact).  Closure bonds (a, b, input length): broken if |d_ab - length| > bond_tol.  n_broken, and
 *     max_bond_dev = the largest |d_ab - length| (0: no closure bonds).  Passes if n_broken == 0.
 *   passed: bit 0 = check 1, bit 1 = check 2, bit 2 = both (pk_valid).
 * Every reduction is a minimum, a maximum or an integer count, so a frame's outputs are bitwise the same alone or in any batch.
 * A frame with a non-finite or out-of-range (|x| > 1e4) coordinate (or a radius outside (0, 4]) gets counts of -1, NaN floats,
 * worst_pair (-1, -1), passed 0 and an all-zero res_clash row.  Limits: M_g <= 8192, n_res_g <= 16384, exclusion lists of at
 * most 32 atoms (max_* above them: DBFR_ERR_ARG).  Static atoms are not limited.                                            */
typedef struct {
  int32_t        n_group;
  int32_t        n_frame;        /* frame_ptr[G]: one workgroup per frame                                                   */
  const int32_t* frame_ptr;      /* [G+1] first frame of every group; per-frame outputs are indexed by frame                */
  const int32_t* pocket_ptr;     /* [G+1] first pocket atom of every group in pocket_rad / _col / _rank (M_g atoms per frame) */
  const int64_t* pocket_pos_off; /* [G] frame k of g at rows pocket_pos_off[g] + k M_g of pocket_pos                         */
  const float*   pocket_pos;     /* [rows, 3]                                                                               */
  const float*   pocket_rad;     /* [pocket_ptr[G]] radii in (0, 4]                                                         */
  const int32_t* pocket_col;     /* [pocket_ptr[G]] residue column, 0 .. n_res_g - 1                                        */
  const int32_t* pocket_rank;    /* [pocket_ptr[G]] position of the atom in its group's movable list, -1 = not movable      */
  const int32_t* static_ptr;     /* [G+1] static atoms of every group in static_pos / _rad / _col, or NULL = none             */
  const float*   static_pos;     /* [static_ptr[G], 3] in the frame of pocket_pos                                           */
  const float*   static_rad;
  const int32_t* static_col;
  const int32_t* mov_ptr;        /* [G+1] movable atoms of every group                                                      */
  const int32_t* mov_atom;       /* [mov_ptr[G]] pocket atom index (0 .. M_g - 1) of every movable atom, ascending per group */
  const int32_t* excl_ptr;       /* [mov_ptr[G] + 1] CSR over the movable atoms of all groups into excl                      */
  const int32_t* excl;           /* receptor atom indices b of the group, ascending within a list, at most 32 per list       */
  const int32_t* closure_ptr;    /* [G+1] closure bonds of every group                                                      */
  const int32_t* closure_ab;     /* [closure_ptr[G], 2] receptor atom indices                                               */
  const float*   closure_len;    /* [closure_ptr[G]] length in the input structure (A)                                      */
  const int32_t* res_ptr;        /* [G+1]: n_res_g = res_ptr[g+1] - res_ptr[g]                                               */
  const int64_t* res_off;        /* [G] frame k of g writes res_clash[res_off[g] + k n_res_g ...]                            */
  int32_t        max_pocket;     /* host-known maxima over the groups (<= 8192, 32, 16384)                                  */
  int32_t        max_excl;
  int32_t        max_res;
  int32_t        cand_cap;       /* partner candidates gathered in LDS per round, 0 = 1024 (same bits whatever the value; tests;
                                    256 .. 1024)                                                                            */
  const void*    host;           /* NULL, or a dbfr_pocket_check_in whose pointers are HOST copies of the same arrays (the two
                                    position arrays are not read): every list length, atom index, residue column and radius is
                                    then validated before the launch (DBFR_ERR_ARG)                                          */
} dbfr_pocket_check_in;

typedef struct {
  float   clash_ratio;           /* (0, 10], default 0.75                                                                   */
  float   bond_tol;              /* A, >= 0, default 0.3                                                                    */
  int32_t max_clashes;           /* >= 0, default 0                                                                         */
} dbfr_pocket_check_opts;

typedef struct {                 /* device arrays; any may be NULL                                                          */
  int32_t* n_clash;              /* [n_frame, 3] sc_sc, sc_bb, sc_static                                                    */
  float*   min_ratio;            /* [n_frame]                                                                               */
  int32_t* worst_pair;           /* [n_frame, 2]                                                                            */
  uint8_t* res_clash;            /* [sum_g F_g n_res_g]                                                                     */
  int32_t* n_broken;             /* [n_frame]                                                                               */
  float*   max_bond_dev;         /* [n_frame]                                                                               */
  int32_t* passed;               /* [n_frame]                                                                               */
} dbfr_pocket_check_out;

/* One launch for the whole batch.  opts NULL = defaults.                                                                    */
int dbfr_pocket_check(const dbfr_pocket_check_in* in, const dbfr_pocket_check_opts* opts, const dbfr_pocket_check_out* out,
                      void* hip_stream);

/* ---- Solvent-accessible and buried surface area of poses (csrc/sasa.hip; docs/sasa.md): Shrake-Rupley with integer results.  A
 * batch of G groups (one group = the frames of one ligand in one complex), group g holding F_g frames of N_g ligand heavy atoms
 * (L), M_g pocket atoms per frame and S_g static receptor atoms shared by its frames (R; receptor atom b of a frame: pocket atom
 * b for b < M_g, static atom b - M_g otherwise) and n_res_g residue columns.  Atom i has a radius r_i in (0, 4], the expanded
 * radius R_i = r_i + probe, an integer area weight w_i > 0 (n_points w_i <= 2^21), a polar flag and, in R, a residue column.
 * points = n_points unit vectors u_k.  Point k of atom i is buried by atom c != i when |(x_i - x_c) + R_i u_k| < R_c; the
 * difference x_i - x_c is formed first and no absolute point position is ever formed (float32, every operation rounded).
 *   lig_free   points of a ligand atom buried by no other ligand atom                  (the free ligand in the pose's conformation)
 *   lig_bound  points of a ligand atom buried by no other atom of L u R
 *   buried_b   points of receptor atom b buried by at least one ligand atom and by no other receptor atom; summed with weights
 *              this is SASA(receptor alone) - SASA(receptor in the complex)
 *   res_buried [frame, residue column] = sum over the residue's atoms of buried_b w_b
 *   totals     [frame, 6] = sum lig_free w, sum lig_bound w, the same two over the polar ligand atoms, sum buried_b w_b over R,
 *              the same over the polar receptor atoms.  An area is a sum in units of 2^-12 A^2 when w = round(4 pi R^2 / n 4096).
 * Every reduction is an integer sum, so a frame's outputs are bitwise the same alone, in any batch and for any cand_cap.  A frame
 * with a non-finite or out-of-range (|x| > 1e4) coordinate (or a radius outside (0, 4]) gets -1 in every count and total and an
 * all-zero res_buried row.  Limits: N_g <= 256, M_g <= 8192, n_res_g <= 16384 (max_* above them: DBFR_ERR_ARG); n_points a
 * multiple of 64 in [64, 512]; probe in [0, 2].  Static atoms are not limited.                                              */
typedef struct {
  int32_t        n_group;
  int32_t        n_frame;        /* frame_ptr[G]: one workgroup per frame                                                   */
  const int32_t* frame_ptr;      /* [G+1] first frame of every group; totals are indexed by frame                           */
  const int32_t* lig_ptr;        /* [G+1] first atom of every group in lig_rad / _w / _polar (N_g atoms per frame, may be 0)  */
  const int64_t* lig_pos_off;    /* [G] frame k of g at rows lig_pos_off[g] + k N_g of lig_pos, lig_free and lig_bound        */
  const float*   lig_pos;        /* [rows, 3]                                                                               */
  const float*   lig_rad;        /* [lig_ptr[G]] radii in (0, 4]                                                            */
  const int32_t* lig_w;          /* [lig_ptr[G]] area weight of one point, > 0                                              */
  const uint8_t* lig_polar;      /* [lig_ptr[G]] 1 = polar (N, O)                                                           */
  const int32_t* pocket_ptr;     /* [G+1] first pocket atom of every group in pocket_rad / _w / _col / _polar (may be 0 atoms) */
  const int64_t* pocket_pos_off; /* [G] frame k of g at rows pocket_pos_off[g] + k M_g of pocket_pos                         */
  const float*   pocket_pos;     /* [rows, 3]                                                                               */
  const float*   pocket_rad;
  const int32_t* pocket_w;
  const int32_t* pocket_col;     /* residue column, 0 .. n_res_g - 1                                                        */
  const uint8_t* pocket_polar;
  const int32_t* static_ptr;     /* [G+1] static atoms of every group in static_pos / _rad / _w / _col / _polar, or NULL = none */
  const float*   static_pos;     /* [static_ptr[G], 3] in the frame of lig_pos                                              */
  const float*   static_rad;
  const int32_t* static_w;
  const int32_t* static_col;
  const uint8_t* static_polar;
  const int32_t* res_ptr;        /* [G+1]: n_res_g = res_ptr[g+1] - res_ptr[g]                                               */
  const int64_t* res_off;        /* [G] frame k of g writes res_buried[res_off[g] + k n_res_g ...]                           */
  const float*   points;         /* [n_points, 3] unit vectors                                                              */
  int32_t        n_points;       /* 64, 128, ..., 512                                                                       */
  int32_t        max_lig;        /* host-known maxima over the groups (<= 256, 8192, 16384)                                 */
  int32_t        max_pocket;
  int32_t        max_res;
  int32_t        cand_cap;       /* receptor atoms kept in LDS per frame, 0 = 1536 (same bits whatever the value; tests;
                                    256 .. 2048); the atoms beyond it are read from memory                                  */
  const void*    host;           /* NULL, or a dbfr_sasa_in whose pointers are HOST copies of the same arrays (the two frame
                                    position arrays are not read): every count, residue column, radius, weight and point is
                                    then validated before the launch (DBFR_ERR_ARG)                                          */
} dbfr_sasa_in;

typedef struct {
  float probe;                   /* A, [0, 2], default 1.4                                                                  */
} dbfr_sasa_opts;

typedef struct {                 /* device arrays; any may be NULL                                                          */
  int32_t* lig_free;             /* [rows of lig_pos]                                                                       */
  int32_t* lig_bound;            /* [rows of lig_pos]                                                                       */
  int32_t* res_buried;           /* [sum_g F_g n_res_g]                                                                     */
  int64_t* totals;               /* [n_frame, 6]                                                                            */
} dbfr_sasa_out;

/* One launch for the whole batch.  opts NULL = defaults.                                                                    */
int dbfr_sasa(const dbfr_sasa_in* in, const dbfr_sasa_opts* opts, const dbfr_sasa_out* out, void* hip_stream);

/* ---- Cavity volume and ligand fill of each pose's pocket (csrc/cavity.hip; docs/cavity.md): the LIGSITE-style definition of
 * docs/sites.md evaluated per frame.  Groups, frames, ligand (L) and receptor (R) atoms as in dbfr_sasa_in.  Per group a lattice
 * of 32^3 points q = spacing * (grid_lo + (i, j, k)) (float32), shared by the group's frames.
 *   P          points with |q - x_a|^2 < fp32((r_a + probe)^2) for a receptor atom a; q - x_a is formed first, per component, and
 *              the squares are summed (dx^2 + dy^2) + dz^2 (float32, every operation rounded)
 *   b(q)       the lines (3 axes, 4 body diagonals) that reach a P point within T_e = floor(ray_length / (spacing |e|)) steps in
 *              both senses; 0 at P points; a point outside the box is solvent
 *   cavity     solvent points with b >= min_buried
 *   covered    points with |q - x_l|^2 < fp32(r_l^2) for a ligand atom l
 *   C          the union of the 6-connected components of cavity points that hold a covered point
 *   mouth      points of C with a 6-neighbour that is solvent and no cavity point (a neighbour outside the box counts)
 *   lining     receptor atoms with |q - x_a|^2 <= fp32(lining_cutoff^2) for a q in C (bit 0 of the residue's byte), and for a q in
 *              C that is not covered (bit 1: the free room)
 *   totals     [frame, 12] = covered points, those in P, those that are cavity points (filled; all in C), those that are solvent
 *              and no cavity point, |C|, mouth points, sum b over C, sum b over the filled points, lining atoms, lining atoms
 *              flagged polar, ligand atoms whose own nearest lattice index rint(x / spacing) (float32) lies outside the box,
 *              |C and C of frame ref_frame[g]| (-1 without a reference frame)
 * Every result is an integer OR, count or sum: a frame's outputs are bitwise the same alone, in any batch and in any group
 * order.  A frame with a non-finite or out-of-range (|x| > 1e4) coordinate (or a radius outside (0, 4]) gets -1 in every total,
 * an all-zero lining row, zero masks and a zero burial grid.  Limits: N_g <= 256, M_g <= 8192, n_res_g <= 16384 (max_* above
 * them: DBFR_ERR_ARG); grid_lo in [-4096, 4064].  Static atoms are not limited.                                              */
typedef struct {
  int32_t        n_group;
  int32_t        n_frame;        /* frame_ptr[G]: one workgroup per frame                                                   */
  const int32_t* frame_ptr;      /* [G+1] first frame of every group; totals and masks are indexed by frame                 */
  const int32_t* lig_ptr;        /* [G+1] first atom of every group in lig_rad (N_g atoms per frame, may be 0)              */
  const int64_t* lig_pos_off;    /* [G] frame k of g at rows lig_pos_off[g] + k N_g of lig_pos                              */
  const float*   lig_pos;        /* [rows, 3]                                                                               */
  const float*   lig_rad;        /* [lig_ptr[G]] radii in (0, 4]                                                            */
  const int32_t* pocket_ptr;     /* [G+1] first pocket atom of every group in pocket_rad / _col / _polar (may be 0 atoms)   */
  const int64_t* pocket_pos_off; /* [G] frame k of g at rows pocket_pos_off[g] + k M_g of pocket_pos                        */
  const float*   pocket_pos;     /* [rows, 3]                                                                               */
  const float*   pocket_rad;
  const int32_t* pocket_col;     /* residue column, 0 .. n_res_g - 1                                                        */
  const uint8_t* pocket_polar;
  const int32_t* static_ptr;     /* [G+1] static atoms of every group in static_pos / _rad / _col / _polar, or NULL = none  */
  const float*   static_pos;     /* [static_ptr[G], 3] in the frame of lig_pos                                              */
  const float*   static_rad;
  const int32_t* static_col;
  const uint8_t* static_polar;
  const int32_t* res_ptr;        /* [G+1]: n_res_g = res_ptr[g+1] - res_ptr[g]                                               */
  const int64_t* res_off;        /* [G] frame k of g writes lining[res_off[g] + k n_res_g ...]                              */
  const int32_t* grid_lo;        /* [G, 3] lattice index of the box's first point (x y z), each in [-4096, 4064]            */
  const int32_t* ref_frame;      /* [G] the launch's frame whose C every frame of the group is compared with (a frame of the
                                    same group), -1 = none; NULL = no group has one                                         */
  int32_t        max_lig;        /* host-known maxima over the groups (<= 256, 8192, 16384)                                 */
  int32_t        max_pocket;
  int32_t        max_res;
  const void*    host;           /* NULL, or a dbfr_cavity_in whose pointers are HOST copies of the same arrays (the position
                                    and polar arrays are not read): every count, residue column, radius, lattice corner and
                                    reference frame is then validated before the launch (DBFR_ERR_ARG)                      */
} dbfr_cavity_in;

typedef struct {
  float   spacing;               /* A, [0.75, 2], default 1.0                                                               */
  float   probe;                 /* A, [0, 4], default 1.2                                                                  */
  float   ray_length;            /* A, [spacing, 31 spacing], default 8.0                                                   */
  float   lining_cutoff;         /* A, [0, 6], default 4.0                                                                  */
  int32_t min_buried;            /* [1, 7], default 6                                                                       */
} dbfr_cavity_opts;

typedef struct {                 /* device arrays; totals, lining, masks and burial may be NULL                             */
  int32_t*  totals;              /* [n_frame, 12]                                                                           */
  uint8_t*  lining;              /* [sum_g F_g n_res_g]                                                                     */
  uint32_t* masks;               /* [n_frame, 2, 32 (k), 32 (j)]: C, and C AND covered; bit i of a word = x index i         */
  uint8_t*  burial;              /* [n_frame, 32 (k), 32 (j), 32 (i)] b(q), 4-byte aligned                                  */
  void*     workspace;           /* dbfr_pose_cavity_workspace_bytes device bytes, read and written when ref_frame is given */
  size_t    workspace_bytes;
} dbfr_cavity_out;

int dbfr_pose_cavity_workspace_bytes(const dbfr_cavity_in* in, size_t* bytes);
/* k_pose_cavity, one workgroup per frame, then (with ref_frame) k_cavity_common on the same stream.  opts NULL = defaults.   */
int dbfr_pose_cavity(const dbfr_cavity_in* in, const dbfr_cavity_opts* opts, const dbfr_cavity_out* out, void* hip_stream);

/* ---- Holo-pocket recovery of apo / AF2 docking (csrc/apoholo.hip; docs/apoholo.md): what the reference's pair_spatial_metrics
 * (DiffBindFR/utils/apo_holo.py) measures between a holo crystal structure and the docked apo structure, for every pose.
 *
 * Global sequence alignment, host only (no GPU call), library threads over a ragged batch of n_pair sequence pairs.  Scoring is
 * match 1, mismatch 0, gaps 0: the score is the length of the longest common subsequence.  Residue codes outside 0..19 match
 * nothing.  With S[i][j] the score of a[0..i) against b[0..j) the traceback runs from (na, nb): take the pair (i-1, j-1) when
 * a[i-1] == b[j-1] and S[i][j] == S[i-1][j-1] + 1, else step i-1 when S[i-1][j] == S[i][j], else step j-1.
 * a_to_b[a_ptr[p] + i] = index in sequence b of pair p of the identical residue a[i] is paired with, or -1.  na nb above
 * DBFR_ALIGN_MAX_CELLS (2^26) is refused with DBFR_ERR_ARG.  n_threads <= 0: one per core, at most 16.                     */
#define DBFR_ALIGN_MAX_CELLS (1 << 26)
int dbfr_seq_align(int32_t n_pair, const int32_t* a_ptr, const int32_t* a, const int32_t* b_ptr, const int32_t* b,
                   int32_t* a_to_b, int32_t* score, int32_t n_threads);

/* Binding-site selection on the device, one launch for a ragged batch of n_pair structures: residue r of pair p is flagged when
 * any of its atoms lies within cutoff (sqrt(d2) <= cutoff, float32) of any ligand atom.  Atoms are whatever the caller lists
 * (heavy atoms and, for selection only, hydrogens), each with the residue it belongs to.  All pointers are device pointers.  */
typedef struct {
  int32_t        n_pair;
  const int32_t* atom_ptr;       /* [n_pair+1] atoms of every pair in atom_pos / atom_res                                    */
  const float*   atom_pos;       /* [atom_ptr[n_pair], 3]                                                                   */
  const int32_t* atom_res;       /* [atom_ptr[n_pair]] residue of the atom, 0 .. n_res_p - 1 (others are skipped)             */
  const int32_t* lig_ptr;        /* [n_pair+1] ligand atoms of every pair in lig_pos                                         */
  const float*   lig_pos;        /* [lig_ptr[n_pair], 3]                                                                    */
  const int32_t* res_ptr;        /* [n_pair+1] residues of every pair in `site`                                              */
  int32_t        n_res;          /* res_ptr[n_pair] (host-known): the bytes of `site`                                        */
  int32_t        max_atoms;      /* host-known maximum of the atoms of one pair                                             */
  float          cutoff;         /* A, (0, 100]                                                                             */
} dbfr_holo_site_in;
/* site: [res_ptr[n_pair]] bytes, zeroed by the call on the stream, 1 = site residue.                                        */
int dbfr_holo_site(const dbfr_holo_site_in* in, uint8_t* site, void* hip_stream);

/* The per-frame metrics.  A batch of G groups (one group = one complex with its holo/apo pair record), group g holding F_g frames
 * (poses), S_g site residues, R_g sampled pocket rows per frame, H_g holo ligand atoms, N_g atoms of the pose's own ligand
 * (0 = none) and n_perm_g automorphisms of it.  Site residue s has a type, a `matched` flag, its holo atom14 coordinates and mask in
 * the frame of the poses, and the frame's residue: pocket row site_row[s] of the frame when site_row[s] >= 0, else the static
 * atoms apo14[s]; frame_mask[s] is the atom14 mask of that residue.  Unmatched rows get NaN / 0 everywhere.
 *   pair_dist [group, s, 14, H]  |holo atom - holo ligand atom| (float32) of every SCORED pair, -1 elsewhere.  Scored: s matched,
 *              the atom present in holo_mask and frame_mask, distance < radius.  Formed once per group; every frame reads it.
 *   plddt_den [group, s]  scored pairs of s                                      (int32)
 *   lddt_den  [group]     sum of plddt_den                                       (int32)
 *   sc_rmsd   [frame, s]  sqrt(mean |holo - frame|^2) over atom14 slots 4..13 (the heavy atoms but N, CA, C, O), NaN when the two
 *              present-atom sets differ or are empty; sc_sq_sum / sc_n [frame]: the sum of squares and atom count pooled over s
 *   chi       [frame, s, 4], altchi [frame, s, 2]  chi1..chi4 of the frame's residue (IUPAC sign, radians, the library's chi atom
 *              table) and the alternative naming: altchi1 of VAL (CG2), altchi2 of ASP (OD2), LEU, PHE, TYR (CD2); NaN elsewhere
 *   dchi      [frame, s, 4]  |chi - holo_chi| wrapped into [0, pi]; where the alternative exists and is defined, the minimum of
 *              that and |altchi - holo_chi| wrapped
 *   plddt_num [frame, s]  sum over the scored pairs of how many of |d_holo - d_frame| < 0.5, 1, 2, 4 hold, d_frame measured from
 *              the frame's atom to the HOLO ligand atom                           (int32)
 *   lddt_num  [frame]     the same summed over s with d_frame measured to atom perms[p][h] of the pose's own ligand, maximum
 *              over p; -1 when N_g != H_g                                          (int32)
 * Float sums run in a fixed order and counts are integers: a frame's outputs are bitwise the same alone, in any batch and in any
 * frame order.  A frame with a non-finite or |x| > 1e4 coordinate gets -1 in every count and NaN in every float.
 * Limits (DBFR_ERR_ARG beyond them): H_g, N_g <= 256; 14 R_g <= 8192 pocket atoms; S_g <= 512; automorphisms are not limited. */
#define DBFR_HOLO_MAX_LIG 256
#define DBFR_HOLO_MAX_POCKET 8192
#define DBFR_HOLO_MAX_SITE 512
typedef struct {
  int32_t        n_group;
  int32_t        n_frame;        /* frame_ptr[G]: one workgroup per frame                                                   */
  const int32_t* frame_ptr;      /* [G+1] first frame of every group; per-frame outputs are indexed by frame                 */
  const int32_t* site_ptr;       /* [G+1] first site residue of every group in the per-residue arrays below                  */
  const int32_t* site_aatype;    /* [site_ptr[G]] 0..19 (others: no chi angles)                                             */
  const int32_t* site_row;       /* [site_ptr[G]] pocket row of the residue, or -1: apo14 for every frame                    */
  const uint8_t* site_matched;   /* [site_ptr[G]]                                                                           */
  const float*   holo14;         /* [site_ptr[G], 14, 3]                                                                    */
  const uint8_t* holo_mask;      /* [site_ptr[G], 14]                                                                       */
  const float*   apo14;          /* [site_ptr[G], 14, 3] read where site_row < 0                                            */
  const uint8_t* frame_mask;     /* [site_ptr[G], 14]                                                                       */
  const float*   holo_chi;       /* [site_ptr[G], 4] chi1..chi4 of the holo residue, NaN where undefined                     */
  const int64_t* site_off;       /* [G] frame k of g writes its per-residue outputs at rows site_off[g] + k S_g              */
  const int32_t* res_ptr;        /* [G+1]: R_g = res_ptr[g+1] - res_ptr[g]                                                   */
  const int64_t* pocket_off;     /* [G] frame k of g at rows pocket_off[g] + k R_g of pocket                                 */
  const float*   pocket;         /* [rows, 14, 3]                                                                           */
  const int32_t* hlig_ptr;       /* [G+1] holo ligand atoms of every group in hlig                                           */
  const float*   hlig;           /* [hlig_ptr[G], 3]                                                                        */
  const int64_t* pair_off;       /* [G] first float of group g in pair_dist (S_g 14 H_g floats)                              */
  const int32_t* lig_ptr;        /* [G+1]: N_g = lig_ptr[g+1] - lig_ptr[g]                                                   */
  const int64_t* lig_off;        /* [G] frame k of g at rows lig_off[g] + k N_g of lig                                       */
  const float*   lig;            /* [rows, 3] the poses' own ligand atoms                                                   */
  const int32_t* perm_ptr;       /* [G+1] first automorphism of every group (n_perm_g >= 1 where N_g == H_g > 0)              */
  const int64_t* perm_off;       /* [G] first int of group g in perms                                                       */
  const int32_t* perms;          /* group by group [n_perm_g, N_g]: holo ligand atom h is compared with pose atom perms[p][h] */
  int32_t        max_site;       /* host-known maxima over the groups (<= 512, 585, 256)                                    */
  int32_t        max_res;
  int32_t        max_lig;        /* over N_g and H_g                                                                        */
  const void*    host;           /* required: a dbfr_holo_metrics_in whose pointers are HOST copies of the index arrays (the
                                    coordinate, mask, type and chi arrays are not read): every count, pocket row, offset and
                                    automorphism entry is validated before the launches (DBFR_ERR_ARG)                       */
} dbfr_holo_metrics_in;

typedef struct {
  float radius;                  /* A, (0, 100], default 6.0: holo pairs below it are scored                               */
} dbfr_holo_metrics_opts;

typedef struct {                 /* device arrays; all but pair_dist may be NULL                                             */
  float*   pair_dist;            /* [sum_g S_g 14 H_g] written by the first launch, read by the second                       */
  int32_t* plddt_den;            /* [site_ptr[G]]                                                                           */
  int32_t* lddt_den;             /* [G]                                                                                     */
  float*   sc_rmsd;              /* [sum_g F_g S_g]                                                                         */
  float*   sc_sq_sum;            /* [n_frame]                                                                               */
  int32_t* sc_n;                 /* [n_frame]                                                                               */
  float*   chi;                  /* [sum_g F_g S_g, 4]                                                                      */
  float*   altchi;               /* [sum_g F_g S_g, 2]                                                                      */
  float*   dchi;                 /* [sum_g F_g S_g, 4]                                                                      */
  int32_t* plddt_num;            /* [sum_g F_g S_g]                                                                         */
  int32_t* lddt_num;             /* [n_frame]                                                                               */
} dbfr_holo_metrics_out;

/* Two launches for the whole batch: the pairs of every group, then every frame.  opts NULL = defaults.                      */
int dbfr_holo_metrics(const dbfr_holo_metrics_in* in, const dbfr_holo_metrics_opts* opts, const dbfr_holo_metrics_out* out,
                      void* hip_stream);

/* ---- Pocket conformational states of the sampled poses (csrc/pocketstates.hip; docs/pocketstates.md): the receptor across the
 * frames of a complex.  A batch of G groups (one group = one complex), group g holding F_g frames of R_g pocket rows (atom14,
 * pocket-centred) with one residue type, atom14 mask and `counted` flag (res_mask) per row.  With ref_last the last frame of a group
 * is a reference frame (the input structure): it takes part in the matrices, not in the statistics over the poses.
 *   side-chain distance of frames i < j at residue s: A_s = the present atom14 slots 4..13, n_s = |A_s|,
 *     q_id = sum_{a in A_s} |x_i[a] - x_j[a]|^2, q_sw the same against x_j[swap(a)] (the 180-degree renamings of ASP, GLU, PHE, TYR;
 *     formed where the type's swap is not the identity and maps A_s onto itself), each ONE serial float32 sum in slot order,
 *     q_s = min(q_id, q_sw), D_s = sqrtf(q_s / n_s).  A residue with n_s = 0 or res_mask = 0 does not count.
 *   dist_max    [F, F]  max_s D_s                              worst_res [F, F] the lowest s attaining it (int32)
 *   dist_pooled [F, F]  sqrtf(sum_s q_s / sum_s n_s), both sums serial in ascending s
 *     Only i < j is computed and mirrored: the matrices equal their transposes bit for bit.  The diagonal is an exact 0 with
 *     worst_res -1; where no residue counts the distances are 0 and worst_res is -1.
 *   chi [frame, s, 4]   chi1..chi4 in radians (IUPAC sign, the chi atom table of dbfr_holo_metrics), NaN where undefined
 *   rot [frame, s]      sum_k bin_k 3^k over the chi the type defines, a = chi in degrees: not pi-periodic: a wrapped into [0, 360),
 *                       bin 0 = [0, 120), 1 = [120, 240), 2 = [240, 360); pi-periodic: a folded into [-45, 135) by 180, bin 0 =
 *                       [-45, 45), 1 = [45, 135).  -1 when a chi the type defines is NaN; 0 for a type without chi.
 *   per (group, s), over the usable pose frames: n_rot (distinct codes >= 0), top_rot / top_count (the most common code, ties to the
 *     smaller code; -1 / 0 of none), ref_rot / ref_count (the reference frame's code and the poses sharing it; -1 / 0 without one),
 *     mob_max = max_{i<j} D_s, mob_sq = sum_{i<j} llrintf(min(q_s / n_s, 4096) 2^20) (int64), dev_ref_max = max_i D_s(i, ref);
 *     0 / -1 for a residue that does not count (the rotamer statistics read res_mask only).
 *   n_used [G] the usable pose frames; frame_ok [n_frame] 1 = usable.
 * A frame is unusable when a present atom (all 14 slots) of a counted residue is non-finite or beyond 1e4 A: its row and column
 * (diagonal included) are NaN in both matrices with worst_res -1, its chi NaN, its rot -1, and no statistic reads it.  Maxima and
 * integer sums are exact in any order and no float sum depends on the tiling: a group's outputs are bitwise the same alone, in any
 * batch, in any group order and at any tile size.  Limits (DBFR_ERR_ARG): 512 frames per group (reference included), 585 pocket
 * rows, 65 535 groups.  A group whose device-side counts exceed max_frame / max_res gets NaN / -1 / 0 in its own slices only.   */
#define DBFR_PKS_MAX_FRAME 512
#define DBFR_PKS_MAX_RES 585
typedef struct {
  int32_t        n_group;
  int32_t        n_frame;        /* frame_ptr[G]                                                                            */
  const int32_t* frame_ptr;      /* [G+1] first frame of every group; per-frame outputs are indexed by frame                 */
  const int32_t* res_ptr;        /* [G+1] first pocket row of every group in aatype / atom14_mask / res_mask and the per-residue outputs */
  const int64_t* pocket_off;     /* [G] sum_{h<g} F_h R_h: frame k of g at rows pocket_off[g] + k R_g of pocket, chi and rot    */
  const float*   pocket;         /* [rows, 14, 3]                                                                           */
  const int32_t* aatype;         /* [res_ptr[G]] 0..19 (others: no chi, no swap)                                            */
  const uint8_t* atom14_mask;    /* [res_ptr[G], 14]                                                                        */
  const int8_t*  res_mask;       /* [res_ptr[G]] 0 = the residue does not count; NULL = every residue counts                  */
  const int8_t*  ref_last;       /* [G] 1 = the group's last frame is its reference frame; NULL = opts.ref_last for every group */
  const int64_t* pair_off;       /* [G] sum_{h<g} F_h^2: where the group's matrices start                                    */
  int32_t        max_frame;      /* host-known maxima over the groups (<= 512, <= 585)                                      */
  int32_t        max_res;
  const void*    host;           /* required: a dbfr_pocket_states_in whose pointers are HOST copies of frame_ptr, res_ptr, pocket_off,
                                    pair_off and (where given) ref_last: every count and offset is validated before the launches  */
} dbfr_pocket_states_in;

typedef struct {
  int32_t ref_last;              /* 0 / 1 for every group when in.ref_last is NULL (default 0)                               */
  int32_t tile_rows;             /* frames per LDS tile, 0 = 16, at most 16 (same bits whatever the value; for tests)         */
} dbfr_pocket_states_opts;

typedef struct {                 /* device arrays, all required                                                             */
  float*   dist_max;             /* [sum_g F_g^2]                                                                           */
  float*   dist_pooled;          /* [sum_g F_g^2]                                                                           */
  int32_t* worst_res;            /* [sum_g F_g^2]                                                                           */
  float*   chi;                  /* [sum_g F_g R_g, 4]                                                                      */
  int32_t* rot;                  /* [sum_g F_g R_g]                                                                         */
  int32_t* n_rot;                /* [res_ptr[G]], as the seven below                                                        */
  int32_t* top_rot;
  int32_t* top_count;
  int32_t* ref_rot;
  int32_t* ref_count;
  float*   mob_max;
  int64_t* mob_sq;
  float*   dev_ref_max;
  int32_t* n_used;               /* [G]                                                                                     */
  uint8_t* frame_ok;             /* [n_frame] written by the first launch, read by the other two                             */
} dbfr_pocket_states_out;

/* Three launches for the whole batch on the stream: every frame (chi, rot, frame_ok), every group (the rotamer statistics), every
 * (pair tile, group) (the matrices and the mobility statistics, which the call zeroes first).  opts NULL = defaults.             */
int dbfr_pocket_states(const dbfr_pocket_states_in* in, const dbfr_pocket_states_opts* opts, const dbfr_pocket_states_out* out,
                       void* hip_stream);

/* ---- In-place Gaussian shape and feature overlap of conformations (csrc/shapesim.hip; docs/shapesim.md): a pose against a known
 * ligand, or the poses of different ligands against each other, with no atom correspondence.  A molecule m has N_m heavy atoms, each
 * with a Gaussian width alpha and flag bits (1 donor, 2 acceptor, 4 hydrophobe), LG_m groups in the lgrp layout of the
 * interaction fingerprints: kind 0 ring / 1 cation / 2 anion, six local atom indices padded with -1, then 0; and one width
 * color_alpha for its feature points.  A cloud c is molecule cloud_mol[c] at the N_m position rows from cloud_pos_off[c] on, expanded into points
 * (x, y, z, alpha, kind):
 *   kind 0 shape      every atom, its own alpha           kind 3 cation / 4 anion / 5 ring   the centroid of every group of that
 *   kind 1 donor      every atom with bit 1, color_alpha                                     kind (serial float32 sum in list order,
 *   kind 2 acceptor   every atom with bit 2, color_alpha                                     divided by the count), color_alpha
 *   kind 6 hydrophobe every atom with bit 4, color_alpha
 * Two points of the same kind contribute (float32, every operation rounded)
 *     dx = xa - xb (dy, dz alike), d2 = (dx dx + dy dy) + dz dz, s = aa + ab, q = (aa ab) / s, c = PI_F / s,
 *     v = ((8 c) sqrtf(c)) expf(-(q d2)),      term = llrint((double)v 4294967296.0)      (int64, units of 2^-32 A^3)
 * which has the same bits with the two points swapped; points of different kinds contribute nothing and there is no cutoff.
 * O[a, b, k] is the integer sum of the terms of kind k over all point pairs of the clouds a and b:
 *   self_fixed [n_cloud, 7]  O[c, c, .]
 *   pair_fixed [n_pair, 7]   set s is the block A_s x B_s of clouds (a_cloud[a_ptr[s] ..], b_cloud[b_ptr[s] ..]; b_ptr NULL: B_s = A_s for
 *                            every set); the pair (i, j) of set s is row pair_off[s] + i |B_s| + j
 *   tanimoto   [n_pair, 2]   with S = channel 0, C = the channels 1..6 summed as integers, in double and rounded once:
 *                            S_ab / ((S_aa + S_bb) - S_ab), and the same on C (NaN when C_aa + C_bb == 0)
 *   dist       [n_pair]      1 - sim, sim = T_shape when C_aa == 0 or C_bb == 0, else (1 - w) T_shape + w T_color in double, w =
 *                            (double)color_weight; an exact 0 at i == j of a set with B_s = A_s
 * Every sum is an integer sum: a pair's bits do not depend on the batch, its position, the tiling (b_tile) or the side a cloud is on.
 * A cloud with a non-finite coordinate or one beyond 1e4 A gets INT64_MIN in its self row and in every pair row it takes part in, and
 * NaN in the floats; nothing else is touched.  tanimoto and dist read self_fixed, which must then be given.  Limits (DBFR_ERR_ARG):
 * 1..256 atoms and at most 32 groups per molecule, at most 1 024 points per cloud, alpha and color_alpha in [0.1, 1e4], at most 4 096
 * clouds on either side of a set, at most 65 535 sets.                                                                            */
#define DBFR_SHAPE_KINDS 7
#define DBFR_SHAPE_MAX_ATOMS 256
#define DBFR_SHAPE_MAX_GROUPS 32
#define DBFR_SHAPE_MAX_POINTS 1024
#define DBFR_SHAPE_MAX_SIDE 4096
typedef struct {
  int32_t        n_mol;
  int32_t        n_cloud;
  const int32_t* mol_atom_ptr;   /* [n_mol+1] first atom of every molecule in alpha / flags                                  */
  const float*   alpha;          /* [mol_atom_ptr[n_mol]] kappa / r^2                                                        */
  const uint8_t* flags;          /* [mol_atom_ptr[n_mol]] bit 0 donor, 1 acceptor, 2 hydrophobe                              */
  const float*   color_alpha;    /* [n_mol] the width of the molecule's feature points                                       */
  const int32_t* mol_grp_ptr;    /* [n_mol+1] first group of every molecule                                                  */
  const int32_t* grp;            /* [mol_grp_ptr[n_mol], 8]: kind, 6 local atom indices (-1 padded, at least 1), 0             */
  const int32_t* cloud_mol;      /* [n_cloud] the molecule of every cloud                                                    */
  const int64_t* cloud_pos_off;  /* [n_cloud] first row of the cloud in pos                                                  */
  const float*   pos;            /* [n_pos_row, 3]                                                                           */
  const int32_t* a_ptr;          /* [n_set+1] into a_cloud                                                                   */
  const int32_t* a_cloud;        /* [a_ptr[n_set]] cloud indices                                                             */
  const int32_t* b_ptr;          /* [n_set+1] into b_cloud; NULL: B = A for every set (b_cloud is not read)                    */
  const int32_t* b_cloud;
  const int64_t* pair_off;       /* [n_set] sum_{t<s} |A_t| |B_t|                                                            */
  int32_t        n_set;
  int32_t        max_a;          /* host-known maxima of |A_s| and |B_s| (<= 4 096)                                          */
  int32_t        max_b;
  int64_t        n_pos_row;      /* rows of pos                                                                              */
  const void*    host;           /* required: a dbfr_shape_in whose pointers are HOST copies of every array but pos: every count and
                                    index is validated before the launches                                                    */
} dbfr_shape_in;

typedef struct {
  float   color_weight;          /* w in [0, 1] (default 0.5)                                                                */
  int32_t b_tile;                /* clouds of B per workgroup, 0 = 32 (same bits whatever the value; for tests)               */
} dbfr_shape_opts;

typedef struct {                 /* device arrays, any may be NULL (tanimoto / dist need self_fixed)                          */
  int64_t* self_fixed;           /* [n_cloud, 7]                                                                             */
  int64_t* pair_fixed;           /* [n_pair, 7]                                                                              */
  float*   tanimoto;             /* [n_pair, 2] shape, colour                                                                */
  float*   dist;                 /* [n_pair]                                                                                 */
} dbfr_shape_out;

/* Two launches for the whole batch on the stream: every cloud (self_fixed), every (tile of B, cloud of A, set).  opts NULL =
 * defaults.                                                                                                                   */
int dbfr_shape_overlap(const dbfr_shape_in* in, const dbfr_shape_opts* opts, const dbfr_shape_out* out, void* hip_stream);

/* ---- Checks of poses against cofactors, metal ions and waters (csrc/hetero.hip; docs/hetero.md).  A batch of G groups (one
 * group = the frames of one ligand in one complex), group g holding F_g frames of N_g ligand heavy atoms (L), H_g hetero atoms
 * shared by its frames, M_g pocket atoms per frame and S_g static receptor atoms shared by its frames (receptor atom b of a
 * frame: pocket atom b for b < M_g, static atom b - M_g otherwise; read for water bridges only) and n_res_g residue columns.
 * A ligand atom has a vdW radius, a covalent radius and flag bits (1 polar, 2 coordinating); a hetero atom a class (0 organic
 * cofactor, 1 inorganic cofactor, 2 water), a vdW radius, a covalent radius and a metal flag; a receptor atom a polar flag and
 * a residue column.  d_ah = sqrt of the sum of the squared coordinate differences (float32, every operation rounded);
 * R_ah = vdW + vdW for the classes 0 and 2, covalent + covalent for class 1.  Per hetero atom h: d_h = min_a d_ah, a_h the
 * lowest a attaining it, rho_h = min_a d_ah / R_ah.
 * Per frame and class c ([n_frame, 3]):
 *   min_dist    min d_h over the class, min_ratio  min rho_h (+inf: the class is empty), worst  the lowest h attaining it (-1)
 *   n_clash     pairs with d_ah / R_ah < clash_ratio
 *   vol_lig     lattice points {grid k, k in Z^3} strictly within vol_scale[c] vdW_a of some ligand atom
 *   vol_overlap those of them strictly within vol_scale[c] vdW_h of some hetero atom of class c
 * Events, one per hetero atom, bits or'ed: 1 CLASH rho_h < clash_ratio; 2 DISPLACED a water with d_h < displace_dist; 4 COORD a
 * metal with n_coord_h >= 1 coordinating ligand atoms at d_ah <= metal_dist; 8 LIGPOLAR a water that is not DISPLACED with a
 * polar ligand atom at d_ah <= hbond_dist (p_h: the nearest, lowest index on a tie); 16 BRIDGE LIGPOLAR and a polar receptor
 * atom at d <= hbond_dist of the water (b_h: the nearest, lowest index on a tie).  An atom with any of the bits 1, 2, 4, 16 is
 * emitted, in hetero-atom order: event_i {h, bits, a_h, n_coord_h, p_h or -1, b_h or -1}, event_f {d_h, rho_h, d(h, b_h) or
 * NaN}; slots not used hold -1 / NaN; n_event is the true count even above max_event.
 * Per frame: n_displaced / n_bridge / n_coord = the hetero atoms with that bit; passed: bits 0..2 min_ratio[c] >= clash_ratio
 * for c = 0, 1, 2, bits 3..5 vol_overlap[c] <= vol_overlap_max[c] vol_lig[c], bit 6 all six (an empty class passes both).
 * Every reduction is a min, a max or an integer sum: a frame's outputs are bitwise the same alone, in any batch and for any
 * cand_cap.  A frame with a non-finite or out-of-range (|x| > 1e4) coordinate or a radius outside (0, 4] gets NaN / -1 in every
 * output and passed 0.  Limits (DBFR_ERR_ARG beyond them): N_g <= 256, M_g <= 8192, n_res_g <= 16384, max_event in [1, 256];
 * hetero and static atoms are not limited.                                                                                  */
typedef struct {
  int32_t        n_group;
  int32_t        n_frame;        /* frame_ptr[G]: one workgroup per frame                                                   */
  const int32_t* frame_ptr;      /* [G+1] first frame of every group; per-frame outputs are indexed by frame                 */
  const int32_t* lig_ptr;        /* [G+1] first atom of every group in lig_rad / _cov / _flags (N_g atoms per frame)          */
  const int64_t* lig_pos_off;    /* [G] frame k of g at rows lig_pos_off[g] + k N_g of lig_pos                               */
  const float*   lig_pos;        /* [rows, 3]                                                                               */
  const float*   lig_rad;        /* [lig_ptr[G]] vdW radii in (0, 4]                                                        */
  const float*   lig_cov;        /* [lig_ptr[G]] covalent radii in (0, 4]                                                   */
  const uint8_t* lig_flags;      /* [lig_ptr[G]] 1 = polar (N, O), 2 = coordinating (N, O, S)                                */
  const int32_t* het_ptr;        /* [G+1] first hetero atom of every group in het_pos / _rad / _cov / _class / _metal (may be 0) */
  const float*   het_pos;        /* [het_ptr[G], 3] in the frame of lig_pos                                                 */
  const float*   het_rad;        /* vdW radii in (0, 4]                                                                     */
  const float*   het_cov;        /* covalent radii in (0, 4]                                                                */
  const uint8_t* het_class;      /* 0 organic cofactor, 1 inorganic cofactor, 2 water                                       */
  const uint8_t* het_metal;      /* 1 = a metal                                                                             */
  const int32_t* pocket_ptr;     /* [G+1] first pocket atom of every group in pocket_polar / _col (may be 0 atoms)            */
  const int64_t* pocket_pos_off; /* [G] frame k of g at rows pocket_pos_off[g] + k M_g of pocket_pos                         */
  const float*   pocket_pos;     /* [rows, 3]                                                                               */
  const uint8_t* pocket_polar;   /* 1 = polar (N, O)                                                                        */
  const int32_t* pocket_col;     /* residue column, 0 .. n_res_g - 1 (validated; the caller names b_h's residue with it)     */
  const int32_t* static_ptr;     /* [G+1] static atoms of every group in static_pos / _polar / _col, or NULL = none           */
  const float*   static_pos;     /* [static_ptr[G], 3] in the frame of lig_pos                                              */
  const uint8_t* static_polar;
  const int32_t* static_col;
  const int32_t* res_ptr;        /* [G+1]: n_res_g = res_ptr[g+1] - res_ptr[g]                                               */
  int32_t        max_lig;        /* host-known maxima over the groups (<= 256, 8192, 16384)                                 */
  int32_t        max_pocket;
  int32_t        max_res;
  int32_t        cand_cap;       /* hetero atoms kept in LDS for the lattice passes, 0 = 1024 (same bits whatever the value;
                                    tests; 1 .. 1024); with more candidates the passes read the hetero atoms from memory    */
  const void*    host;           /* NULL, or a dbfr_hetero_check_in whose pointers are HOST copies of the same arrays (the three
                                    position arrays are not read): every count, class, radius and residue column is then
                                    validated before the launch (DBFR_ERR_ARG)                                              */
} dbfr_hetero_check_in;

typedef struct {
  float   clash_ratio;           /* 0.75                                                                                    */
  float   displace_dist;         /* A, 2.0                                                                                  */
  float   metal_dist;            /* A, 2.8                                                                                  */
  float   hbond_dist;            /* A, 3.5, in (0, 8]                                                                       */
  float   grid;                  /* A, 0.25, in [0.05, 1]                                                                   */
  float   vol_scale[3];          /* per class, 0.8 / 0.5 / 0.5, each in (0, 2]                                              */
  float   vol_overlap_max[3];    /* per class, 0.075                                                                        */
  int32_t max_event;             /* K, 32, in [1, 256]                                                                      */
} dbfr_hetero_check_opts;

typedef struct {                 /* device arrays; any may be NULL                                                          */
  float*   min_dist;             /* [n_frame, 3]                                                                            */
  float*   min_ratio;            /* [n_frame, 3]                                                                            */
  int32_t* worst;                /* [n_frame, 3]                                                                            */
  int32_t* n_clash;              /* [n_frame, 3]                                                                            */
  int32_t* vol_lig;              /* [n_frame, 3]                                                                            */
  int32_t* vol_overlap;          /* [n_frame, 3]                                                                            */
  int32_t* n_displaced;          /* [n_frame]                                                                               */
  int32_t* n_bridge;             /* [n_frame]                                                                               */
  int32_t* n_coord;              /* [n_frame]                                                                               */
  int32_t* passed;               /* [n_frame]                                                                               */
  int32_t* event_i;              /* [n_frame, K, 6]                                                                         */
  float*   event_f;              /* [n_frame, K, 3]                                                                         */
  int32_t* n_event;              /* [n_frame]                                                                               */
} dbfr_hetero_check_out;

/* One launch for the whole batch.  opts NULL = defaults.                                                                    */
int dbfr_hetero_check(const dbfr_hetero_check_in* in, const dbfr_hetero_check_opts* opts, const dbfr_hetero_check_out* out,
                      void* hip_stream);

/* ---- Polar hydrogens and angle-checked hydrogen bonds of poses (csrc/hydrogens.hip; docs/hydrogens.md).  The batch layout is
 * that of the sibling analyses: G groups, group g holding F_g frames of N_g ligand heavy atoms, M_g pocket atoms per frame and
 * S_g static receptor atoms (receptor atom b: pocket atom b for b < M_g, static atom b - M_g otherwise) and n_res_g residue
 * columns.  A group has NHL_g ligand hydrogens with NRL_g ligand rotors (indices: ligand atoms) and NHR_g pocket hydrogens with
 * NRR_g pocket rotors (indices: receptor atoms; the parent is a pocket atom and the hydrogens are sorted by parent).
 * A hydrogen is {p, q, r, kind, rotor or -1, flags (1: the parent is N, O or S), 0, 0} and four floats:
 *   kind 0 CARRY   e1 = unit(q - p), e2 = unit((r - p) - ((r - p).e1) e1), e3 = e1 x e2, H = p + f0 e1 + f1 e2 + f2 e3
 *   kind 1 BISECT  H = p + f0 unit(unit(p - q) + unit(p - r))
 *   kind 2 AMIDE, kind 3 ROTOR  e1 = unit(p - q), e2 = unit((r - q) - ((r - q).e1) e1), e3 = e1 x e2,
 *                  H = p + f0 e1 + f1 ((c f2 - s f3) e2 + (s f2 + c f3) e3): f0 = -l cos(theta), f1 = l sin(theta), (f2, f3) = the
 *                  cosine and sine of the dihedral (r-q-p-H) at k = 0, (c, s) = those of k steps (1, 0 for AMIDE)
 * A rotor is {first hydrogen, n_h in 1..3 (consecutive hydrogens), K in 1..12, 0} and the cosine and sine of one step; (c, s)
 * of k steps are k complex products with the step, from (1, 0), every one rounded.  Candidates of a rotor with parent p: for
 * a ligand rotor the receptor acceptors A with d(p, A) <= hb_dist, for a pocket rotor the ligand acceptors and the receptor
 * acceptors of another residue column within the same distance.  k = the lowest k attaining  min_k min_j,A d(H_kj, A); 0
 * without candidates.
 * Acceptors: ligand atoms with lig_acc != 0, receptor atoms with bit 0 of meta[0] (meta = {acceptor + 256 column, 3 heavy
 * neighbours as receptor atoms or -1}).  A bond (D, H, A) across the interface: d(D, A) <= hb_dist, d(H, A) <= hb_h_dist,
 * cos(D-H..A) <= cos(hb_dha_angle), cos(y-A..H) <= cos(hb_acc_angle) for every listed neighbour y of A; one bond per (D, A),
 * with the passing hydrogen of smallest d(H, A) (the lowest index on a tie).  Bonds are listed ligand donors first, then by D,
 * then by A: bond_i {side (0: the ligand donates), D, H, A}, bond_f {d(D, A), d(H, A), cos(D-H..A)}; slots not used hold -1 /
 * NaN and n_bond is the true count even above max_bond.  counts {side-0 bonds, side-1 bonds, ligand hydrogens with flag 1 that
 * are the hydrogen of no bond}; res_bits: 1 the residue donates to the ligand, 2 it accepts from it.  Minima carry their index,
 * sums are integer: a frame's bytes are the same alone, in any batch and for any cand_cap.  A frame with a non-finite or
 * |x| > 1e4 coordinate gets counts and n_bond of -1 and zeros elsewhere (-1 / NaN in the bond list).  Limits (DBFR_ERR_ARG
 * beyond them): N_g <= 256, NHL_g <= 256, NRL_g <= 64, NHR_g <= 4096, n_res_g <= 16384, max_bond in [1, 64].                */
typedef struct {
  int32_t        n_group;
  int32_t        n_frame;
  const int32_t* frame_ptr;      /* [G+1]                                                                                   */
  const int32_t* lig_ptr;        /* [G+1] first atom of every group in lig_acc / lig_nbr                                     */
  const int64_t* lig_pos_off;    /* [G] frame k of g at rows lig_pos_off[g] + k N_g of lig_pos                               */
  const float*   lig_pos;        /* [rows, 3]                                                                               */
  const uint8_t* lig_acc;        /* [lig_ptr[G]] 1 = acceptor                                                               */
  const int32_t* lig_nbr;        /* [lig_ptr[G], 3] heavy neighbours, -1 padded                                             */
  const int32_t* lh_ptr;         /* [G+1] first ligand hydrogen of every group in lh_i / lh_f                                */
  const int32_t* lh_i;           /* [lh_ptr[G], 8]                                                                          */
  const float*   lh_f;           /* [lh_ptr[G], 4]                                                                          */
  const int32_t* lrot_ptr;       /* [G+1] first ligand rotor of every group in lrot_i / lrot_f                               */
  const int32_t* lrot_i;         /* [lrot_ptr[G], 4]                                                                        */
  const float*   lrot_f;         /* [lrot_ptr[G], 2]                                                                        */
  const int64_t* lh_out_off;     /* [G] frame k of g at rows lh_out_off[g] + k NHL_g of out.lig_h                            */
  const int64_t* lk_off;         /* [G] frame k of g at lk_off[g] + k NRL_g of out.lig_k                                     */
  const int32_t* pocket_ptr;     /* [G+1] first pocket atom of every group in pocket_meta                                   */
  const int64_t* pocket_pos_off; /* [G]                                                                                     */
  const float*   pocket_pos;     /* [rows, 3]                                                                               */
  const int32_t* pocket_meta;    /* [pocket_ptr[G], 4]                                                                      */
  const int32_t* static_ptr;     /* [G+1], or NULL = no static atoms                                                        */
  const float*   static_pos;     /* [static_ptr[G], 3]                                                                      */
  const int32_t* static_meta;    /* [static_ptr[G], 4]                                                                      */
  const int32_t* rh_ptr;         /* [G+1] first pocket hydrogen of every group in rh_i / rh_f                                */
  const int32_t* rh_i;           /* [rh_ptr[G], 8]                                                                          */
  const float*   rh_f;           /* [rh_ptr[G], 4]                                                                          */
  const int32_t* rrot_ptr;       /* [G+1]                                                                                   */
  const int32_t* rrot_i;         /* [rrot_ptr[G], 4]                                                                        */
  const float*   rrot_f;         /* [rrot_ptr[G], 2]                                                                        */
  const int64_t* rh_out_off;     /* [G] frame k of g at rows rh_out_off[g] + k NHR_g of out.rec_h                            */
  const int64_t* rk_off;         /* [G] frame k of g at rk_off[g] + k NRR_g of out.rec_k                                     */
  const int32_t* res_ptr;        /* [G+1]: n_res_g = res_ptr[g+1] - res_ptr[g]                                               */
  const int64_t* res_off;        /* [G] frame k of g at res_off[g] + k n_res_g of out.res_bits                               */
  int32_t        max_lig;        /* host-known maxima over the groups (<= 256, 256, 64, 4096, 16384)                        */
  int32_t        max_lig_h;
  int32_t        max_lig_rot;
  int32_t        max_rec_h;
  int32_t        max_res;
  int32_t        cand_cap;       /* receptor acceptors kept in LDS, 0 = 2048 (same bytes whatever the value; tests; 1 .. 2048);
                                    with more the kernel reads the receptor atoms from memory                               */
  const void*    host;           /* NULL, or a dbfr_hydrogens_in of HOST copies of the index arrays (the position arrays are not
                                    read): every count, index, kind and rotor is then validated before the launch           */
} dbfr_hydrogens_in;

typedef struct {
  float   hb_dist;               /* A, 3.5, in (0, 8]                                                                       */
  float   hb_h_dist;             /* A, 2.5                                                                                  */
  float   hb_dha_angle;          /* degrees, 120, in [0, 180]                                                               */
  float   hb_acc_angle;          /* degrees, 90, in [0, 180]                                                                */
  int32_t max_bond;              /* 64, in [1, 64]                                                                          */
} dbfr_hydrogens_opts;

typedef struct {                 /* device arrays, all required                                                             */
  float*   lig_h;                /* [rows, 3] ligand hydrogen positions                                                     */
  float*   rec_h;                /* [rows, 3] pocket hydrogen positions                                                     */
  int32_t* lig_k;                /* [rows] the chosen k of every ligand rotor                                               */
  int32_t* rec_k;                /* [rows] the chosen k of every pocket rotor                                               */
  int32_t* counts;               /* [n_frame, 3]                                                                            */
  int32_t* n_bond;               /* [n_frame]                                                                               */
  int32_t* bond_i;               /* [n_frame, max_bond, 4]                                                                  */
  float*   bond_f;               /* [n_frame, max_bond, 3]                                                                  */
  uint8_t* res_bits;             /* [rows] one word per (frame, residue column)                                             */
} dbfr_hydrogens_out;

/* One launch for the whole batch.  opts NULL = defaults.                                                                    */
int dbfr_hydrogens(const dbfr_hydrogens_in* in, const dbfr_hydrogens_opts* opts, const dbfr_hydrogens_out* out, void* hip_stream);

/* ---- Per-residue and per-atom decomposition of the Vina inter-molecular energy of poses (csrc/decompose.hip;
 * docs/decompose.md).  The batch layout is that of the sibling analyses: G groups, group g holding F_g frames of N_g ligand
 * heavy atoms, M_g pocket atoms per frame and S_g static receptor atoms (receptor atom b: pocket atom b for b < M_g, static atom
 * b - M_g otherwise).  Every ligand and receptor atom carries an XS type (the codes of dbfr_vina_in: 0..15, 17 = Met_D; 16 and
 * any value outside 0..17 takes part in no term) and every receptor atom a column in 0 .. n_col_g - 1: the caller numbers the
 * protein's residues first and the hetero residues (cofactors, ions, waters: static atoms) after them.
 * For every pair (ligand atom i, receptor atom b) with r^2 < cutoff^2 the five weighted fp32 terms t_k(i, b) are those of
 * dbfr_vina_score (gauss1, gauss2, repulsion, hydrophobic, hbond), each rounded once to an integer q_k = rint(t_k 2^36).
 *   col_fixed  [sum_g F_g n_col_g, 5]  sum of q_k over the pairs of the column's atoms; frame k of g at rows col_off[g] + k n_col_g
 *   atom_fixed [sum_g F_g N_g, 5]      sum of q_k over the pairs of the ligand atom; frame k of g at rows lig_pos_off[g] + k N_g
 *   totals_fixed [n_frame, 6]          sum of q_k over all pairs, and the sum of the five (E_inter)
 *   col_terms / atom_terms / totals    the same values in kcal/mol: (float)((double)sum 2^-36)
 * Every sum is an integer sum: a frame's outputs are bitwise the same alone, in any batch and at any position in it, and the
 * columns and the atoms of a frame both add up to its totals exactly in the integer outputs.  A column without an atom in reach
 * holds exact zeros.  A frame with a non-finite or out-of-range (|x| > 1e4) coordinate, or (without `host`) a column outside
 * 0 .. n_col_g - 1, gets NaN in every float row and INT64_MIN in every integer row.  Limits (DBFR_ERR_ARG beyond them):
 * N_g in 1 .. 256, n_col_g <= 16384; receptor atoms are not limited.                                                          */
typedef struct {
  int32_t        n_group;
  int32_t        n_frame;        /* frame_ptr[G]: one workgroup per frame                                                   */
  const int32_t* frame_ptr;      /* [G+1] first frame of every group; totals are indexed by frame                            */
  const int32_t* lig_ptr;        /* [G+1] first atom of every group in lig_type (N_g atoms per frame)                        */
  const int64_t* lig_pos_off;    /* [G] frame k of g at rows lig_pos_off[g] + k N_g of lig_pos and of atom_terms: the groups'
                                    rows follow each other without gaps                                                     */
  const float*   lig_pos;        /* [rows, 3]                                                                               */
  const int8_t*  lig_type;       /* [lig_ptr[G]] XS types                                                                   */
  const int32_t* pocket_ptr;     /* [G+1] first pocket atom of every group in pocket_type / _col (may be 0 atoms)             */
  const int64_t* pocket_pos_off; /* [G] frame k of g at rows pocket_pos_off[g] + k M_g of pocket_pos                         */
  const float*   pocket_pos;     /* [rows, 3]                                                                               */
  const int8_t*  pocket_type;
  const int32_t* pocket_col;
  const int32_t* static_ptr;     /* [G+1] static atoms of every group in static_pos / _type / _col, or NULL = none            */
  const float*   static_pos;     /* [static_ptr[G], 3] in the frame of lig_pos                                              */
  const int8_t*  static_type;
  const int32_t* static_col;
  const int32_t* col_ptr;        /* [G+1]: n_col_g = col_ptr[g+1] - col_ptr[g]                                               */
  const int64_t* col_off;        /* [G] frame k of g at rows col_off[g] + k n_col_g of col_terms: without gaps, as lig_pos_off */
  int32_t        max_lig;        /* host-known maxima over the groups (<= 256, 16384)                                       */
  int32_t        max_col;
  const void*    host;           /* NULL, or a dbfr_vina_decompose_in whose pointers are HOST copies of the same arrays (positions
                                    and types are not read): every count, row offset and column is then validated before
                                    the launch (DBFR_ERR_ARG)                                                               */
} dbfr_vina_decompose_in;

typedef struct {
  float cutoff;                  /* A, 8.0, in (0, 16]                                                                      */
} dbfr_vina_decompose_opts;

typedef struct {                 /* device arrays; any but col_fixed may be NULL                                            */
  float*   col_terms;            /* [sum_g F_g n_col_g, 5]                                                                  */
  float*   atom_terms;           /* [sum_g F_g N_g, 5]                                                                      */
  float*   totals;               /* [n_frame, 6]                                                                            */
  int64_t* col_fixed;            /* [sum_g F_g n_col_g, 5]: the column sums are accumulated here                             */
  int64_t* atom_fixed;           /* [sum_g F_g N_g, 5]                                                                      */
  int64_t* totals_fixed;         /* [n_frame, 6]                                                                            */
} dbfr_vina_decompose_out;

/* One launch for the whole batch.  opts NULL = defaults.                                                                    */
int dbfr_vina_decompose(const dbfr_vina_decompose_in* in, const dbfr_vina_decompose_opts* opts, const dbfr_vina_decompose_out* out,
                        void* hip_stream);

/* ---- XTC trajectory encoding (csrc/xtc.hip; docs/trajectory.md).  A batch of n_frame frames, each written into one of n_file
 * files; a file is the frames listed for it, in frame order, with one atom map.  Atom k of a frame is atom_map[map_ptr[m] + k]
 * (m = file_map[frame_file[f]]) of source frame s = frame_src[f]:
 *   0 <= code < 0x40000000        ligand atom code of lig[s]                                   (+ center)
 *   code = DBFR_XTC_POCKET(r, a)  atom14 slot a of pocket row r of pos14[s]                    (+ center)
 *   code = DBFR_XTC_STATIC(m)     static_pos[m], absolute
 * (the centre added in float32).  Every coordinate x (A) goes through the chain a PDB file and an XTC writer apply:
 *   q3 = rint((double)x * 1000) ("%8.3f"), xp = (float)((double)q3 / 1000) (a reader's float32), xn = xp * 0.1f (nm),
 *   p = xn * precision, int = (int)(float)(p +- 0.5) (+ for xn >= 0),
 * and frames are written in the XTC layout of libxdrfile's xdrfile_compress_coord_float (GROMACS xdr3dfcoord): header
 * (1995, natoms, step, time, box[9], natoms), then <= 9 atoms: 3 natoms floats xn, else precision, minint[3], maxint[3],
 * smallidx, nbytes and the bit stream.  Big-endian throughout.  step = first_step + frame_step[f], time = step_time * dt.
 * Refused with DBFR_ERR_ARG after the launch (the call synchronises the stream): |p +- 0.5| > INT_MAX - 2, a range
 * maxint - minint >= INT_MAX - 2, a frame whose consecutive atoms are so far apart that the adaptive table index would leave
 * the table (smallidx + 8 >= 73), an index outside its array, frame_file not 0, 1, ... in frame order (every file at least one
 * frame), more atoms than max_atoms.  Limits: n_frame <= 2^20, max_atoms <= 2^20.                                        */
#define DBFR_XTC_POCKET(r, a) (0x40000000 + (r) * 14 + (a))
#define DBFR_XTC_STATIC(m) (-1 - (m))
typedef struct {
  int32_t        n_frame;
  int32_t        n_file;
  int32_t        n_src;          /* source frames in lig / pos14                                                          */
  int32_t        n_lig;          /* ligand atoms per source frame                                                         */
  int32_t        n_res;          /* pocket rows per source frame                                                          */
  int32_t        n_static;
  int32_t        n_map;
  int32_t        max_atoms;      /* host-known bound of every map's length (sizes the workspace and the output)            */
  const float*   lig;            /* [n_src, n_lig, 3] pocket-centred (may be NULL when n_lig == 0)                          */
  const float*   pos14;          /* [n_src, n_res, 14, 3] pocket-centred (may be NULL when n_res == 0)                      */
  const float*   center;         /* [3]                                                                                    */
  const float*   static_pos;     /* [n_static, 3] absolute (may be NULL when n_static == 0)                                 */
  const int32_t* map_ptr;        /* [n_map + 1]                                                                            */
  const int32_t* atom_map;       /* [map_ptr[n_map]] codes                                                                 */
  const int32_t* file_map;       /* [n_file] atom map of every file                                                       */
  const int32_t* frame_file;     /* [n_frame] 0, ..., 0, 1, ..., n_file - 1                                                 */
  const int32_t* frame_src;      /* [n_frame] source frame                                                                 */
  const int32_t* frame_step;     /* [n_frame] step of the frame inside its file (header step = first_step + this)          */
} dbfr_xtc_in;                   /* every pointer a device pointer                                                         */

typedef struct {
  float   precision;             /* default 1000 (<= 0: 1000, like libxdrfile)                                             */
  float   dt;                    /* ps per step, default 1.0: time = step * dt                                             */
  int32_t first_step;            /* default 0                                                                              */
  float   box[9];                /* nm, default zeros (the frame PDBs carry no CRYST1)                                      */
} dbfr_xtc_opts;

/* Workspace bytes of a dbfr_xtc_encode call of this shape and *out_cap, the output bytes to provide (the worst case).   */
int dbfr_xtc_workspace_bytes(const dbfr_xtc_in* in, size_t* bytes, int64_t* out_cap);
/* Encodes every file: out (device, out_cap bytes, 4-byte aligned) receives the file images back to back, offsets (device,
 * [n_file + 1] int64) their byte offsets.  opts NULL = defaults.  Deterministic; a frame's bytes do not depend on the other
 * frames of the launch.  Synchronises the stream (the refusal status).                                                   */
int dbfr_xtc_encode(const dbfr_xtc_in* in, const dbfr_xtc_opts* opts, uint8_t* out, int64_t out_cap, int64_t* offsets,
                    void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- Binding-site detection (csrc/sites.hip; docs/sites.md), LIGSITE-style, for a ragged batch of proteins.
 * Atoms: the atom37 slots with mask > 0 of residues res_ptr[p] .. res_ptr[p+1]; radius = radius[aatype * 37 + slot] (+ probe).
 * Grid: the absolute lattice h Z^3; per protein and axis I = floor(min / h) .. floor(max / h) over its atoms (floor in float64 of
 * the fp32 values), point position h * I in fp32; linear index i + n_x (j + n_y k) (i, j, k = I - lo).  A protein's grid over
 * 1024 points per axis or 2^24 points in all: DBFR_ERR_ARG.
 *   occupied(q)  some atom with |q - x_a|^2 < (r_a + probe)^2 (fp32, every operation rounded);
 *   burial b(q)  over the 3 axes and the 4 body diagonals, the lines that reach an occupied point within T_e = floor(ray_length /
 *                (h |e|)) steps (float64 on the host) in BOTH senses; points off the grid are solvent; 0 at occupied points;
 *   pocket       solvent points with b >= min_buried;
 *   site         a 6-connected component of pocket points, labelled by its smallest linear index.
 * Per site: n_points, score = sum b, idx_sum = sum (i, j, k) (int64), centre = h (lo + idx_sum / n_points) in float64.  Sites with
 * n_points >= min_points are ranked by score (highest first), then label (lowest first); max_sites are kept.  A kept site's
 * lining residues have an atom with |q - x_a| <= lining_cutoff (fp32) for some point q of the site.
 * Integer atomics only (min-label union-find, int32 / int64 sums): a protein's outputs are the same bits alone or in any batch. */
typedef struct {
  float   spacing;               /* h (A), [0.25, 4], default 1.0                                                           */
  float   probe;                 /* A, [0, 4], default 1.2                                                                  */
  float   ray_length;            /* A, [spacing, 255 spacing], default 8.0                                                  */
  float   lining_cutoff;         /* A, [0, 10], default 4.0                                                                 */
  int32_t min_buried;            /* [1, 7], default 6                                                                       */
  int32_t min_points;            /* [1, 2^24], default 30                                                                   */
  int32_t max_sites;             /* [1, 64], default 5                                                                      */
} dbfr_sites_opts;

typedef struct {
  int32_t        n_prot;
  int32_t        n_res;          /* res_ptr[n_prot]                                                                         */
  int64_t        max_points;     /* the workspace's grid-point capacity (the call's total over its proteins), <= 2^30         */
  const int32_t* res_ptr;        /* device [n_prot + 1], 0 .. n_res, not decreasing                                          */
  const int32_t* aatype;         /* device [n_res], 0..20 (others read as 20)                                               */
  const float*   atom37_pos;     /* device [n_res, 37, 3]                                                                   */
  const float*   atom37_mask;    /* device [n_res, 37]                                                                      */
  const float*   radius;         /* device [21, 37] radius of every atom37 slot of every residue type, (0, 4]                 */
} dbfr_sites_in;

typedef struct {                 /* S = opts.max_sites; device arrays unless marked host                                    */
  int32_t* n_sites;              /* [n_prot] sites kept                                                                     */
  int32_t* label;                /* [n_prot, S] linear index of the site's smallest point; -1 for an unused slot               */
  int32_t* n_points;             /* [n_prot, S]                                                                             */
  int32_t* score;                /* [n_prot, S] sum of b                                                                    */
  int64_t* idx_sum;              /* [n_prot, S, 3] (may be NULL)                                                            */
  double*  centre;               /* [n_prot, S, 3] A                                                                        */
  uint8_t* lining;               /* [n_res, S] 1 = residue lines site s of its protein (may be NULL)                          */
  int32_t* grid;                 /* HOST [n_prot, 6]: lo (I of index 0) and n per axis (may be NULL); grid offsets of the
                                    optional grids below: protein p starts at the sum of n_x n_y n_z of proteins < p          */
  uint8_t* occupancy;            /* [total points] 1 = occupied (may be NULL; for tests)                                     */
  uint8_t* burial;               /* [total points] b (may be NULL)                                                          */
  int32_t* labels;               /* [total points] site label of pocket points (every component, kept or not), else -1       */
} dbfr_sites_out;

/* Workspace bytes of a call of in->n_prot proteins and at most in->max_points grid points.                                   */
int dbfr_sites_workspace_bytes(const dbfr_sites_in* in, size_t* bytes);
/* Finds the sites of every protein.  opts NULL = defaults.  Synchronises the stream (res_ptr and the grid sizes are read back);
 * a call whose grids exceed in->max_points fails with DBFR_ERR_CAPACITY before any grid work.                                */
int dbfr_find_sites(const dbfr_sites_in* in, const dbfr_sites_opts* opts, const dbfr_sites_out* out, void* workspace,
                    size_t workspace_bytes, void* hip_stream);

/* Synchronises the stream and returns the device-side status word of the last
 * dbfr_score / dbfr_sample issued with this workspace (DBFR_OK, DBFR_ERR_CAPACITY,
 * DBFR_ERR_NUMERIC).  counters (may be NULL) receives [8] int64: edges of the last
 * step in the order {lig, atom, cross lig<-atom, center, tor, sc_tor, cross atom<-lig, 0}. */
int dbfr_status_sync(void* workspace, void* hip_stream, int64_t* counters);

/* Which matrix instruction carries the 144 x W GEMM of the radial MLP (97-99 % of the arithmetic) in the K=144 convs.
 * All modes produce fp32 results from fp32 weights and fp32 activations:
 *   DBFR_GEMM_F32            v_mfma_f32_16x16x4_f32 (fp32 operands): k_conv / k_conv2;
 *   (1, DBFR_GEMM_SPLIT_BF16 -- three bf16 pieces per operand, six products on v_mfma_f32_16x16x32_bf16, kernel k_conv2r: round 2's default,
 *                            retired with ABI 5 once no conv needed it as a fall-back; the number stays unused)
 *   DBFR_GEMM_SPLIT_F16      every operand cut into TWO fp16 pieces (hi = fp16(x), lo = fp16(x - hi): 23 of fp32's 24 significand
 *                            bits) after an exact power-of-two scaling that keeps the pieces inside fp16's exponent range (W2: per
 *                            tensor-product run, at model creation; activations: per edge, in the kernel), three partial products
 *                            hi*lo + lo*hi + hi*hi on v_mfma_f32_16x16x32_f16, the two small ones and the large one in separate
 *                            fp32 accumulators.  Kernel k_conv2h (csrc/conv2h.hip);
 *                            accuracy table: profiles/r3_split_experiments.txt.
 *   DBFR_GEMM_REDUCE_FIRST   the arithmetic of SPLIT_F16 with the ORDER of the work changed for the rows of lin.3 that feed a scalar (l = 0)
 *                            output irrep (74 % of the rows at depth 3, all rows of the torsion convs): a scalar message element is linear in
 *                            y (x) h (y = the tensor-product input coupled with the harmonics, h = the hidden layer), and so is the scatter over
 *                            the edges of a target node, so Z[t,c,k] = sum_{e -> t} y[e,c] h[e,k] is formed first and the 144 x W GEMM runs
 *                            once per TARGET SEGMENT (the edges of one target inside a chunk = <= 32 consecutive edges and <= 4 targets of one graph), not once per
 *                            edge: 8-10 x fewer matrix instructions for those rows.  Kernel k_convz (csrc/convz.hip); the l = 1 outputs stay
 *                            per edge on k_conv2h.  Every lin.3 output row carries its own power-of-two factor there (no row-depth limit).
 *                            MESSAGE BUFFER in this mode: the scalar columns of a segment's FIRST message row hold the segment's SUM; those of
 *                            its other rows are zero in the buffer dbfr_test_conv2 fills (the hook clears it first) and NOT WRITTEN inside the
 *                            sampler, whose reductions read them of segment-first rows only (vector columns: per edge as before).  Chunks
 *                            are cut per graph, by the graph's own targets: what is summed with what never depends on batch mates.
 * The initial mode is DBFR_GEMM_DEFAULT unless the environment variable DBFR_GEMM (f32 | split_f16 | reduce_first, or the numbers 0 | 3 | 4) says otherwise;
 * any other value -- the retired `split` / `split_l1` / 1 / 2 among them -- makes dbfr_model_create fail with DBFR_ERR_ARG (until ABI 6 it selected the fp32 instruction silently).
 * A workspace is laid out for the mode it was sized in: set the mode before dbfr_workspace_bytes.                       */
#define DBFR_GEMM_F32 0
/* (1 was DBFR_GEMM_SPLIT_BF16, k_conv2r: retired with ABI 5; 2 was DBFR_GEMM_SPLIT_BF16_L1, k_conv2s: retired with ABI 4; the numbers stay unused) */
#define DBFR_GEMM_SPLIT_F16 3
#define DBFR_GEMM_REDUCE_FIRST 4
#define DBFR_GEMM_DEFAULT DBFR_GEMM_REDUCE_FIRST
int dbfr_model_set_gemm(dbfr_model* model, int32_t mode);
/* DBFR_GEMM_SPLIT_F16 holds a weight row to 22 significant bits while the row's largest |w| is within 2^17 of the largest |w| that shares its
 * power-of-two factor -- one per tensor-product run; lin.0: one per matrix.  dbfr_model_create measures every run of every conv; a conv with
 * a deeper row (a trained checkpoint may hold one; seeded weights do not) is packed with one factor per ROW instead, which the kernel takes
 * off the accumulator rows (ABI 5; four more vector instructions per edge block and tile): dbfr_model_rowscaled_convs counts those convs and
 * writes "name:depth;" for each (depth = log2 of the spread that was found).  dbfr_model_fallback_convs counts the convs that even so cannot
 * be held by two fp16 pieces and are served by the fp32-instruction kernel (k_conv2) together with the other convs of their launch (an interaction
 * layer / the two torsion heads): none since ABI 5, unless a bias dwarfs its row by more than 2^48.  names (may be NULL) receives the
 * state_dict prefixes, ';'-terminated each ("atom_conv_layers.3;").                                                                  */
int dbfr_model_rowscaled_convs(const dbfr_model* model, char* names, size_t names_cap);
int dbfr_model_fallback_convs(const dbfr_model* model, char* names, size_t names_cap);
int dbfr_model_get_gemm(const dbfr_model* model);

/* ---- introspection / test hooks */
int         dbfr_abi_version(void);
/* First 16 hex digits of the sha256 over the library's source files at build time (diffbindfr_amd/build.py:
 * source_hash): lets a caller check that a prebuilt libdbfr.so belongs to the source tree next to it.               */
const char* dbfr_build_id(void);
const char* dbfr_last_error(void);
/* Real-basis Wigner-3j tensor the library derives (Racah formula) to self-check
 * the closed forms baked into the kernels; out has (2l1+1)(2l2+1)(2l3+1) doubles. */
int dbfr_wigner3j(int32_t l1, int32_t l2, int32_t l3, double* out);
/* Path table of a conv: n_paths rows of {i1,i2,io,l1,l2,lo,mul1,mulo,w_off} int32
 * + coeff as float bits in column 9. kind: 0..3 layer convs by depth, 4 final_conv,
 * 5 tor convs.  Returns number of paths (<= max_paths) or a negative status.       */
int dbfr_conv_paths(int32_t kind, int32_t* table10, int32_t max_paths, int32_t* weight_numel);
/* Test hook (host code, no GPU): the tile packer of DBFR_GEMM_SPLIT_F16.  frag = n_tiles x [9 k-steps of 16][64 lanes][4] fp32 MFMA
 * fragments (K = 144), bias = n_tiles x 16; out = n_tiles x 9280 bytes: [hi, lo][4 k-steps of 32][64 lanes][8 fp16], then
 * [64 lanes][hi 4 | lo 4 fp16] for the last 16 k, then the 16 bias values (fp32) -- everything multiplied by 2^k, the power of two that
 * puts the largest |value| of these tiles into [2^14, 2^15).  Returns k in *k_out.                                                     */
/* Test hook (GPU): the chunk table k_convz walks, for one flat target-sorted edge list cut every `span` edges as if those were graphs: a chunk =
 * consecutive edges, at most 32 of them and at most four targets.  All pointers are device pointers; scratch holds (max_edges + span - 1) / span + 1
 * ints and receives the first chunk of every span, the total behind them; chunk_es[ch] = first edge, chunk_gl[ch] = number of edges (graph 0). */
int dbfr_test_chunk_table(const int32_t* tgt, const int32_t* n_edges_dev, int32_t max_edges, int32_t span, int32_t* scratch, int32_t cap,
                          int32_t* chunk_es, int32_t* chunk_gl, void* hip_stream);
int dbfr_test_pack_f16_tiles(const float* frag, const float* bias, int32_t n_tiles, void* out, int32_t* k_out);
/* The same packer with one power of two per ROW on top of 2^k (ABI 5; what a conv with rows further apart than 2^17 is packed with):
 * rinv_out [n_tiles x 16] receives 2^-d(row), the factor the kernel takes off the accumulator row; *depth_out the row depth that is left. */
int dbfr_test_pack_f16_rows(const float* frag, const float* bias, int32_t n_tiles, void* out, int32_t* k_out, float* rinv_out, int32_t* depth_out);
/* The range guard of the same packer (host code, no GPU): the largest ROW DEPTH d of these tiles taken as one run -- the row's largest
 * |value| is 2^(15 - d) after the run's factor -- and the limit up to which two fp16 pieces hold a row to 22 significant bits (17): a conv
 * with a deeper row in one of its runs is what dbfr_model_fallback_convs reports.                                                     */
int dbfr_test_pack_f16_depth(const float* frag, const float* bias, int32_t n_tiles, int32_t* depth_out, int32_t* depth_ok_out);
/* Test hook (host code, no GPU): every weight layout model creation builds for ONE conv of `kind` (as dbfr_conv_paths), as digests.  tensors7 = its
 * fc.lin.0 weight and bias, fc.lin.3 weight and bias, batch_norm.mean_shift, affine_weight, affine_bias; numel7 receives their element counts
 * (tensors7 = NULL: nothing else happens, the call returns 0).  rowscale as DBFR_F16_ROWSCALE (0, 1, 2).  The packers run as at model creation:
 * k_conv's layout; for the K = 144 kinds then k_conv2 / k_conv2h's, the same of the vector-output rows alone (kinds 0..3), k_convz's.  Returns the
 * number n of arrays model creation would upload; digests[2i], digests[2i + 1] = byte count and FNV-1a 64 of array i in upload order, digests[2n] =
 * FNV-1a 64 over the non-pointer members of ConvW (with its LNDesc), ConvW2 (both) and ConvZ in declaration order; names (may be NULL) = the arrays'
 * names, ';'-separated; *flags (may be NULL) = per-row factors present: 1 W2rinv, 2 W1rinv, 4 and 8 the same of the vector-output packing.          */
int dbfr_test_pack_conv(int32_t kind, const float* const* tensors7, int32_t rowscale, int64_t* numel7, uint64_t* digests, int32_t digests_cap,
                        char* names, size_t names_cap, int32_t* flags);
/* Profiling hooks: time (ms) spent in the dominant fused conv kernel and the
 * number of launches + edges since the last reset, measured with hip events on
 * the launch stream when profiling is enabled.  conv_flops = algorithmic FLOP
 * (2K(K+W) per edge); ref_form_bytes = HBM bytes the reference's two-kernel form
 * of the same launches would move (4(W+D_in+9)+16 per edge).        */
/* on = 1: events around every fused-conv launch + counters; on = 2: counters only; 0: off.  The launch pattern is the
 * same in all three: every kernel runs on the caller's stream.                                                   */
int dbfr_profile_enable(dbfr_model* m, int32_t on);
int dbfr_profile_read(dbfr_model* m, double* conv_ms, int64_t* conv_launches, double* conv_flops,
                      double* ref_form_bytes, int32_t reset);
/* HBM bytes the FUSED conv has to move for the launches the last dbfr_profile_read reported (read before its reset):
 * 4 (48 + 9 + 3 + 48 + 48 + D_in + D_out) per edge = edge record, two gathered radial-MLP rows, gathered input row, message. */
int dbfr_profile_fused_bytes(const dbfr_model* m, double* fused_form_bytes);
/* Flops the matrix pipe EXECUTED in the launches the last dbfr_profile_read reported: per edge `products` x 2 x 144 x (144 + rows walked) in the per-edge
 * kernels (products: 1 fp32 instruction, 3 two-piece fp16, 6 three-piece bf16), the instructions k_convz issued x 16384 in DBFR_GEMM_REDUCE_FIRST.   */
int dbfr_profile_executed_flops(const dbfr_model* m, double* executed_flops);
/* (ABI 6) Of those, the flops that are NOT padding -- *useful_flops: in DBFR_GEMM_REDUCE_FIRST the hidden layer once per edge (the pair of kernels computes it
 * twice), step A's products over the edges a segment holds (k_convz issues them over all 32 slots of a chunk for each of four segment slots, filled or
 * not), step B's over the segments a unit holds (not the 16-column blocks) and the (path, u) pairs that exist (not the padding of a c tile), times the three
 * partial products; in the per-edge modes the executed flops.  *form_bytes: HBM bytes the form that RUNS has to move for the same launches (the fused
 * form's of dbfr_profile_fused_bytes, but in DBFR_GEMM_REDUCE_FIRST the edge records and gathered rows once per kernel of the pair and the
 * scalar-output message columns once per segment).  Either pointer may be null.                                                          */
int dbfr_profile_useful_flops(const dbfr_model* m, double* useful_flops, double* form_bytes);

/* What the fp16 matrix pipe of the CURRENT device sustains: a bare stream of v_mfma_f32_16x16x32_f16 (the instruction of DBFR_GEMM_SPLIT_F16)
 * with random operands on every compute unit, two waves per SIMD, for `seconds` (0 < seconds <= 60; the rate is taken over the second half,
 * when the firmware has settled the clock at the board's power cap).  *tflops = executed TFLOP/s.  bench.py's roofline.frac_of_sustained
 * divides by it; the instruction's nominal peak (2 500) is reached with all-zero operands only.  Blocks the calling thread.            */
int dbfr_probe_mfma_f16(double seconds, double* tflops, void* hip_stream);

/* Test hook: names (';'-separated) / byte offsets / sizes of the library's internal
 * buffers inside the workspace for this batch shape.  Returns the entry count.       */
int dbfr_workspace_layout(const dbfr_model* m, const dbfr_batch* b, const dbfr_limits* lim, char* names,
                          size_t names_cap, size_t* offsets, size_t* bytes, int32_t max_entries);

/* Unit-test hooks: run ONE fused tensor-product conv (k_conv) / ONE segmented-mean +
 * LayerNorm (k_reduce_ln) of the packed model on caller-supplied device buffers.
 * layer >= 0: interaction layer, family 0 lig, 1 cross_al, 2 atom, 3 cross_la;
 * layer -1 final_conv, -2 tor_bond_conv, -3 sc_tor_bond_conv.                          */
int dbfr_test_conv(dbfr_model* m, int32_t layer, int32_t family, int32_t n_edges, const int32_t* n_edges_dev,
                   const int32_t* tgt, const int32_t* gth, const float* emb, const float* sh, const float* tab1,
                   int32_t ld1, const int32_t* idx1, const float* tab2, int32_t ld2, const int32_t* idx2,
                   const float* x, int32_t ldx, float* msg, void* hip_stream);
/* The same conv through the second-generation kernel k_conv2 (persistent, one W2 stream per CU; K=144 convs only).    */
int dbfr_test_conv2(dbfr_model* m, int32_t layer, int32_t family, int32_t n_edges, const int32_t* n_edges_dev,
                    const int32_t* tgt, const int32_t* gth, const float* emb, const float* sh, const float* tab1,
                    int32_t ld1, const int32_t* idx1, const float* tab2, int32_t ld2, const int32_t* idx2,
                    const float* x, int32_t ldx, float* msg, void* hip_stream);
int dbfr_test_reduce_ln(dbfr_model* m, int32_t layer, int32_t family, const float* msg, const int32_t* row_start,
                        const int32_t* row_cnt, int32_t n_nodes, const float* old, int32_t d_old, float* out,
                        int32_t mode, void* hip_stream);
/* (ABI 6) The same reduction with the message interface of DBFR_GEMM_REDUCE_FIRST: seg_first [n_edges] bytes, 1 = the row's scalar-output columns hold a
 * segment's sum (k_convz stores it in the segment's first row and writes nothing into those columns of the other rows: they are not read, whatever
 * they hold); vector-output columns are per edge.  seg_first == NULL: as dbfr_test_reduce_ln.  K = 144 convs only.                              */
int dbfr_test_reduce_ln2(dbfr_model* m, int32_t layer, int32_t family, const float* msg, const int32_t* row_start,
                         const int32_t* row_cnt, int32_t n_nodes, const float* old, int32_t d_old, float* out,
                         int32_t mode, const uint8_t* seg_first, void* hip_stream);

/* (ABI 7) Test hook: the UPDATE half of one denoise step alone -- what dbfr_sample_range runs after the score network (k_sde_ligand: rigid move,
 * ordered torsion rotations, Kabsch re-alignment; unless no_sc_torsion k_sc_update + k_atom14: chi update, side-chain rebuild, compaction into
 * rec_pos) -- through the very function dbfr_sample_range calls, on caller-supplied scores (tr [G,3], rot [G,3], tor [NTOR], sc_tor [NSC]; device)
 * and ONE step's noise slices (z_tr [G,3], z_rot [G,3], z_tor [NTOR], z_sc [NSC]; device).  Only the g2 / gsdt / dt scalars of `step` are read.
 * Advances b->lig_pos, b->torsion_angle and b->rec_pos in place; atom14_out [NR,14,3] device or NULL.  *err_word_out (device int32, cleared
 * first) receives the status bits the kernels raised (2 = the Kabsch determinant check); nothing is synchronised.                             */
int dbfr_test_sde_step(const dbfr_model* m, const dbfr_batch* b, const dbfr_step* step, const dbfr_scores* scores,
                       const dbfr_noise* z, float* atom14_out, int32_t* err_word_out, void* hip_stream);

/* (ABI 8) Test hooks: the SMALL kernels of the score network alone (tests/test_walk_kernels_gpu.py).  Each runs the launcher the score call runs, with
 * the model's own packed weights and tables, on caller-supplied DEVICE buffers; each refuses a null argument it needs with DBFR_ERR_ARG and
 * synchronises nothing.
 *
 * dbfr_test_time_embed        k_time_embed: temb_out [G,32] = sinusoidal embedding of cfg.emb_scale * t[g].
 * dbfr_test_mlp               k_mlp with weight set `which` (DBFR_MLP_*), in the input mode and with the Gaussian table the score call pairs with
 *                             it: LIG_NODE rows [lig_node(27) | temb[g]], g = row_graph_tab[row]; LIG_EDGE rows [bond_feat[aux] or 0 where
 *                             aux = -1 | temb[g] | gauss(dist)]; ATOM_EDGE, LA_EDGE, CENTER_EDGE rows [temb[g] | gauss(dist)]; TOR_EDGE, SC_EDGE
 *                             rows [gauss(dist)].  Edge rows: g = row_graph_tab[tgt[row]], or row_graph_tab[row] where tgt is NULL (the centre
 *                             set).  n_rows_dev (device int32, or NULL) caps the rows at min(*n_rows_dev, n_rows_max); out [n_rows_max,48],
 *                             rows past the count are not written.  Arguments a mode does not read may be NULL.
 * dbfr_test_atom_encoder      k_atom_encoder: pocket_feat [NA,5] (category ids as floats), atm_batch [NA], temb [G,32] -> out [NA,48].
 * dbfr_test_reduce_ln_layer   k_reduce_ln_layer of interaction layer `layer`: the four reductions of the layer in one launch.  msg, row_start,
 *                             row_cnt: four device pointers each, in the order ligand<-ligand, ligand<-pocket, pocket<-pocket, pocket<-ligand
 *                             (messages [edges, D_out], CSR rows of the NL ligand / NA pocket targets); seg_first: NULL (every column of every
 *                             row is summed), or four flag arrays as dbfr_test_reduce_ln2 takes them.  out_l [NL,D_out] = (pad(old_l [NL,D_in]) +
 *                             LN(mean 0)) + LN(mean 1), out_a likewise from sets 2 and 3.
 * dbfr_test_center_edges      k_center_edges: reads b->G, b->lig_ptr, b->lig_pos only; tgt, gth, dist [NL], sh [NL,9], row_start, row_cnt [G].
 * dbfr_test_trrot             k_trrot: gp [G,12] -> tr_out, rot_out [G,3] with cfg.scale_by_sigma; raises bit 2 of *err_word (device int32, NOT
 *                             cleared by the hook) where an output is not finite.
 * dbfr_test_bond_attr         k_bond_attr in the addressing of head `which` (DBFR_TOR_*): LIGAND attr[k] = nodes[b0[bsel[k]]] + nodes[b1[bsel[k]]],
 *                             SIDECHAIN attr[k] = nodes[b0[2k]] + nodes[b0[2k+1]] (b1, bsel not read); the first 48 columns of rows of `ld` floats.
 * dbfr_test_tor_final         k_tor_final with the head's final MLP: feat [n,96], norm2 [n] -> out [n], times sqrt(norm2) under cfg.scale_by_sigma. */
#define DBFR_MLP_LIG_NODE 0
#define DBFR_MLP_LIG_EDGE 1
#define DBFR_MLP_ATOM_EDGE 2
#define DBFR_MLP_LA_EDGE 3
#define DBFR_MLP_CENTER_EDGE 4
#define DBFR_MLP_TOR_EDGE 5
#define DBFR_MLP_SC_EDGE 6
#define DBFR_TOR_LIGAND 0
#define DBFR_TOR_SIDECHAIN 1
int dbfr_test_time_embed(const dbfr_model* m, const float* t, int32_t G, float* temb_out, void* hip_stream);
int dbfr_test_mlp(const dbfr_model* m, int32_t which, int32_t n_rows_max, const int32_t* n_rows_dev, const float* temb,
                  const int32_t* row_graph_tab, const int32_t* tgt, const int32_t* aux, const float* dist, const float* bond_feat,
                  const float* lig_node, float* out, void* hip_stream);
int dbfr_test_atom_encoder(const dbfr_model* m, const float* pocket_feat, const int32_t* atm_batch, const float* temb, int32_t NA,
                           float* out, void* hip_stream);
int dbfr_test_reduce_ln_layer(const dbfr_model* m, int32_t layer, const float* const* msg, const int32_t* const* row_start,
                              const int32_t* const* row_cnt, const uint8_t* const* seg_first, int32_t NL, int32_t NA, const float* old_l,
                              const float* old_a, float* out_l, float* out_a, void* hip_stream);
int dbfr_test_center_edges(const dbfr_batch* b, int32_t* tgt, int32_t* gth, float* dist, float* sh, int32_t* row_start, int32_t* row_cnt,
                           void* hip_stream);
int dbfr_test_trrot(const dbfr_model* m, const float* gp, const float* temb, const float* tr_sigma, const float* rot_norm, int32_t G,
                    float* tr_out, float* rot_out, int32_t* err_word, void* hip_stream);
int dbfr_test_bond_attr(const dbfr_model* m, int32_t which, const float* nodes, int32_t ld, const int32_t* b0, const int32_t* b1,
                        const int32_t* bsel, int32_t n, float* attr_out, void* hip_stream);
int dbfr_test_tor_final(const dbfr_model* m, int32_t which, const float* feat, const float* norm2, int32_t n, float* out, void* hip_stream);

/* (ABI 9) Test hooks: the kernels of the MDN pose scorer alone (csrc/mdn.hip; tests/test_mdn_kernels_gpu.py).  Each runs the launcher
 * dbfr_mdn_forward runs, on caller-supplied DEVICE buffers; each refuses a null, non-positive or out-of-range argument it needs with
 * DBFR_ERR_ARG and synchronises nothing.  The raw hooks take the caller's own weights (the kernels are generic); the model hooks use the
 * packed weights of a dbfr_mdn_model, BatchNorm folds included.
 *
 * dbfr_test_mdn_lin         k_lin: out[m, 0..N) = act(sum_k X[m,k] W[n,k] + b[n]) (+ res[m,n]), X the concatenation of n_seg <= 4 segments
 *                           (row m of segment i = p[(idx ? idx[m] : m) * ld + 0..w), sum of the w = K); W rows of ldw >= K floats, b or NULL,
 *                           out rows of ldo >= N floats, act 0 none / 1 ReLU / 2 SiLU, res (rows of ldr floats) or NULL.
 * dbfr_test_mdn_gt_attn     k_gt_edge, then k_gt_node: Q, K, V [NL,128], Ep [EL,128], src / dst [EL] (attention over the edges into dst),
 *                           in_ptr [NL+1] / in_edge [EL] (edge ids grouped by dst) -> e_out [EL,128] (NULL: the final layer's form),
 *                           ax [EL,4], h [NL,128].  EL = 0: k_gt_node alone (the edge arrays may be NULL).
 * dbfr_test_mdn_gvp         gvp_run = k_gvp_vec + the scalar k_lin of one GVP: n_vseg <= 3 vector segments (nv vectors of 3 per row, sum = vi),
 *                           n_sseg <= 3 scalar segments (sum of the w = si), wh [h,vi] with h = max(vi, vo) <= 33, wv [vo,h] or NULL (vo = 0),
 *                           ws_w [so, si+h] / ws_b [so] over [scalars | |Vh|] -> vn [M,h], s_out [M,so], v_out [M,vo,3]; act_s as above,
 *                           gate != 0: v *= sigmoid(|v|).
 * dbfr_test_mdn_gvp_ln      k_gvp_ln: s_out = LN(s_in + ds) (ns <= 128; weight lw, bias lb), v_out = (v_in + dv) / sqrt(mean max(|v|^2, 1e-8))
 *                           (nv <= 64 vectors; nv = 0: scalars only); ds / dv NULL = no residual; s_out may equal s_in.
 * dbfr_test_mdn_mean_in     k_mean_in: mean over each node's incoming edge rows ptr[n] .. ptr[n+1] of ms [E,ns] and mv [E,nv3] -> ds [N,ns],
 *                           dv [N,nv3]; a node without rows gets zeros.
 * dbfr_test_mdn_seq_concat  k_seq_concat: out [NR,40] = [node_s [NR,9] | Ws[seq[r]] (31 of a [31,31] table)].
 * dbfr_test_mdn_gt_layer    layer l = 0..5 of the ligand encoder with the model's folded weights: x [NL,128], e [EL,128] -> x_out, e_out
 *                           (e_out is ignored for l = 5).
 * dbfr_test_mdn_head        the mixture-density head: lig_s [NL,128], pro_s [NR,128], lig_pos [NL,3], xyz_full [NR,14,3], lig_ptr / res_ptr
 *                           [B+1] -> Al_out [NL,128] / At_out [NR,128] (either may be NULL), part_out [NL] (double: every ligand atom's sum
 *                           over its graph's residues), score_out [B]; dist_threshold <= 0 = 5.0.
 * The two model hooks take scratch from `workspace`: at least dbfr_mdn_workspace_bytes of a batch with the same B, NL, EL, NR (gt_layer:
 * B = NR = 1; head: EL = 0) and EP = 0.                                                                                                     */
typedef struct { const float* p; int32_t ld; int32_t w; const int32_t* idx; } dbfr_mdn_seg;
typedef struct { const float* p; int32_t nv; const int32_t* idx; } dbfr_mdn_vseg;
int dbfr_test_mdn_lin(const dbfr_mdn_seg* segs, int32_t n_seg, const float* W, int32_t ldw, const float* b, int32_t N, int32_t K, int32_t M,
                      float* out, int32_t ldo, int32_t act, const float* res, int32_t ldr, void* hip_stream);
int dbfr_test_mdn_gt_attn(const float* Q, const float* K, const float* V, const float* Ep, const int32_t* src, const int32_t* dst,
                          const int32_t* in_ptr, const int32_t* in_edge, int32_t NL, int32_t EL, float* e_out, float* ax, float* h,
                          void* hip_stream);
int dbfr_test_mdn_gvp(const dbfr_mdn_vseg* vsegs, int32_t n_vseg, const dbfr_mdn_seg* ssegs, int32_t n_sseg, const float* wh, const float* wv,
                      const float* ws_w, const float* ws_b, int32_t si, int32_t vi, int32_t so, int32_t vo, int32_t act_s, int32_t gate,
                      int32_t M, float* vn, float* s_out, float* v_out, void* hip_stream);
int dbfr_test_mdn_gvp_ln(const float* s_in, const float* ds, int32_t ns, const float* v_in, const float* dv, int32_t nv, const float* lw,
                         const float* lb, int32_t M, float* s_out, float* v_out, void* hip_stream);
int dbfr_test_mdn_mean_in(const float* ms, int32_t ns, const float* mv, int32_t nv3, const int32_t* ptr, int32_t N, float* ds, float* dv,
                          void* hip_stream);
int dbfr_test_mdn_seq_concat(const float* node_s, const int32_t* seq, const float* Ws, int32_t NR, float* out, void* hip_stream);
int dbfr_test_mdn_gt_layer(const dbfr_mdn_model* m, int32_t l, const float* x, const float* e, const int32_t* src, const int32_t* dst,
                           const int32_t* in_ptr, const int32_t* in_edge, int32_t NL, int32_t EL, float* x_out, float* e_out, void* workspace,
                           size_t workspace_bytes, void* hip_stream);
int dbfr_test_mdn_head(const dbfr_mdn_model* m, const float* lig_s, const float* pro_s, const float* lig_pos, const float* xyz_full,
                       const int32_t* lig_ptr, const int32_t* res_ptr, int32_t B, int32_t NL, int32_t NR, float dist_threshold, float* Al_out,
                       float* At_out, double* part_out, float* score_out, void* workspace, size_t workspace_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* DBFR_H */
