"""ctypes binding of libdbfr.so (include/dbfr.h).  Fails loudly when the HIP
library is missing: there is no CPU fallback in the product path."""
import ctypes as C
import os
from functools import lru_cache
from itertools import takewhile

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DBFR_LIB") or os.path.join(HERE, "libdbfr.so")      # DBFR_LIB: developer override (kernel variants)

DBFR_OK = 0
DBFR_ERR_ARG = -1
DBFR_ERR_CAPACITY = -3
ERRORS = {-1: "DBFR_ERR_ARG", -2: "DBFR_ERR_HIP", -3: "DBFR_ERR_CAPACITY", -4: "DBFR_ERR_SELFTEST",
          -5: "DBFR_ERR_NUMERIC"}

i32, f32, vp = C.c_int32, C.c_float, C.c_void_p


class ModelCfg(C.Structure):
    _fields_ = [(n, i32) for n in ("ns", "nv", "sh_lmax", "num_conv_layers", "lig_node_features",
                                   "lig_edge_features", "distance_embed_dim", "sigma_embed_dim")] + \
               [(n, f32) for n in ("emb_scale", "lig_cutoff", "atom_cutoff", "cross_cutoff", "center_max_distance")] + \
               [(n, i32) for n in ("atom_max_neighbors", "lig_max_neighbors", "dynamic_max_cross", "scale_by_sigma",
                                   "no_sc_torsion")]


class Tensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", vp), ("numel", C.c_int64)]


_BATCH_INTS = ("G", "NL", "NA", "NR", "EB", "NTOR", "NSC", "max_nl", "max_na", "max_nr")
_BATCH_PTRS = ("lig_ptr", "lig_node", "lig_pos", "bond_src", "bond_dst", "bond_feat", "bond_ptr", "tor_ptr",
               "tor_bond", "rot_mask", "rot_mask_off", "atm_ptr", "res_ptr", "pocket_feat", "rec_pos", "sequence",
               "backbone_transl", "backbone_rots", "default_frame", "rigid_group_positions", "torsion_angle",
               "atom14_slot", "sc_res_chi", "sc_bond", "sc_ptr")


class Batch(C.Structure):
    _fields_ = [(n, i32) for n in _BATCH_INTS] + [(n, vp) for n in _BATCH_PTRS]


class Limits(C.Structure):
    _fields_ = [("aa_avg_neighbors", i32), ("cross_avg_neighbors", i32)]


class Cond(C.Structure):
    _fields_ = [(n, vp) for n in ("t", "tr_sigma", "rot_score_norm", "tor_score_norm2", "sc_tor_score_norm2")]


class Scores(C.Structure):
    _fields_ = [(n, vp) for n in ("tr", "rot", "tor", "sc_tor")]


class Step(C.Structure):
    _fields_ = [(n, f32) for n in ("t", "dt", "tr_sigma", "rot_score_norm", "tor_score_norm2", "tr_g2", "tr_gsdt",
                                   "rot_g2", "rot_gsdt", "tor_g2", "tor_gsdt", "sc_g2", "sc_gsdt")]


class Noise(C.Structure):
    _fields_ = [(n, vp) for n in ("z_tr", "z_rot", "z_tor", "z_sc")]


class InitTape(C.Structure):
    _fields_ = [(n, vp) for n in ("tor_u", "rot", "tr", "sc_u")]


class PoseMetricsIn(C.Structure):
    _fields_ = [("n_pose", C.c_int32), ("n_frame", C.c_int32), ("n_lig", C.c_int32), ("n_res", C.c_int32),
                ("lig_traj", C.c_void_p), ("prot_traj", C.c_void_p), ("lig_target", C.c_void_p),
                ("atom14_target", C.c_void_p), ("atom14_target_mask", C.c_void_p), ("aatype", C.c_void_p),
                ("n_perm", C.c_int32), ("perms", C.c_void_p), ("heavy_mask", C.c_void_p),
                ("center", C.c_float * 3), ("chi_bound", C.c_float)]


class PoseMetricsOut(C.Structure):
    _fields_ = [("centroid", C.c_void_p), ("sc_rmsd", C.c_void_p), ("chi_rate", C.c_void_p), ("delta_chi", C.c_void_p),
                ("lig_rmsd", C.c_void_p)]


_MDN_PTRS = ("lig_ptr", "lig_node_s", "lig_edge_s", "lig_edge_src", "lig_edge_dst", "lig_in_ptr", "lig_in_edge", "lig_pos",
             "lig_s_in", "res_ptr", "pro_node_s", "pro_node_v", "pro_edge_src", "pro_edge_dst", "pro_in_ptr", "pro_edge_s",
             "pro_edge_v", "pro_seq", "pro_xyz_full")


class MdnBatch(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "NL", "EL", "NR", "EP")] + [(n, C.c_void_p) for n in _MDN_PTRS] + \
               [("dist_threshold", C.c_float)]


class MdnSeg(C.Structure):
    _fields_ = [("p", C.c_void_p), ("ld", C.c_int32), ("w", C.c_int32), ("idx", C.c_void_p)]


class MdnVSeg(C.Structure):
    _fields_ = [("p", C.c_void_p), ("nv", C.c_int32), ("idx", C.c_void_p)]


class SdfTemplate(C.Structure):
    _fields_ = [("n_atoms", C.c_int32), ("header", C.c_char_p), ("atom_tail", C.POINTER(C.c_char_p)), ("trailer", C.c_char_p)]


class PdbTopology(C.Structure):
    _fields_ = [("n_res", C.c_int32), ("aatype", C.c_void_p), ("atom37_pos", C.c_void_p), ("atom37_mask", C.c_void_p),
                ("residue_index", C.c_void_p), ("chain_index", C.c_void_p), ("b_factors", C.c_void_p),
                ("remark", C.c_char_p)]


class VinaIn(C.Structure):
    _fields_ = [("batch", C.c_void_p), ("lig_type", C.c_void_p), ("rec_type", C.c_void_p), ("pair_ptr", C.c_void_p),
                ("pair_ij", C.c_void_p), ("n_pairs", C.c_int32), ("ext_ptr", C.c_void_p), ("ext_pos", C.c_void_p),
                ("ext_type", C.c_void_p), ("max_tor", C.c_int32), ("max_ext", C.c_int32)]


class VinaFlexIn(C.Structure):
    _fields_ = [("base", C.c_void_p)] + [(n, C.c_void_p) for n in ("flex_ptr", "flex_atom", "ftor_ptr", "ftor_bc", "turn_ptr", "turn",
                                                                   "excl_ptr", "excl")] + \
               [(n, C.c_int32) for n in ("n_flex", "n_ftor", "max_flex", "max_ftor", "max_anchor", "max_excl")] + [("host", C.c_void_p)]


class VinaOpts(C.Structure):
    _fields_ = [("max_iters", C.c_int32), ("grad_tol", C.c_float), ("margin", C.c_float)]


class VinaSearchOpts(C.Structure):
    _fields_ = [("chains", C.c_int32), ("n_steps", C.c_int32), ("step_iters", C.c_int32), ("temperature", C.c_float),
                ("amplitude", C.c_float), ("autobox_add", C.c_float), ("random_start", C.c_int32), ("seed", C.c_uint64)]


class PoseRmsdIn(C.Structure):
    _fields_ = [("n_group", C.c_int32), ("pose_ptr", C.c_void_p), ("atom_ptr", C.c_void_p), ("perm_ptr", C.c_void_p),
                ("pos", C.c_void_p), ("perms", C.c_void_p), ("heavy_mask", C.c_void_p), ("max_pose", C.c_int32),
                ("max_atom", C.c_int32), ("path", C.c_int32), ("tile_rows", C.c_int32)]


class ModesOpts(C.Structure):
    _fields_ = [("num_modes", C.c_int32), ("higher_is_better", C.c_int32), ("min_rmsd", C.c_float), ("cluster_rmsd", C.c_float),
                ("energy_range", C.c_float)]


class PoseCheckIn(C.Structure):
    _fields_ = [("n_group", C.c_int32), ("n_frame", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("frame_ptr", "lig_ptr", "lig_pos_off", "lig_pos", "lig_rad", "pocket_ptr", "pocket_pos_off",
                                          "pocket_pos", "pocket_rad", "static_ptr", "static_pos", "static_rad", "pair_ptr", "pair_ij",
                                          "flat_ptr", "flat_atoms", "stereo_ptr", "stereo_atoms", "stereo_sign")] + \
               [(n, C.c_int32) for n in ("max_lig", "max_pair", "max_flat", "max_stereo", "cand_cap")]


class PoseCheckOpts(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("clash_ratio", "max_distance", "vol_scale", "vol_overlap", "internal_ratio", "flat_tol", "grid")]


class PoseCheckOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("min_dist", "min_ratio", "n_clash", "vol_lig", "vol_overlap", "int_min_ratio", "n_int_clash",
                                          "flat_dev", "n_stereo_flip", "passed")]


class InteractionsIn(C.Structure):
    _fields_ = [("n_group", C.c_int32), ("n_frame", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("frame_ptr", "lig_ptr", "lig_pos_off", "lig_pos", "lig_type", "lig_nbr", "lgrp_ptr", "lgrp",
                                          "pocket_ptr", "pocket_pos_off", "pocket_pos", "pocket_meta", "static_ptr", "static_pos",
                                          "static_meta", "rgrp_ptr", "rgrp", "res_ptr", "bits_off")] + \
               [(n, C.c_int32) for n in ("max_lig", "max_lgrp", "max_res")]


class InteractionsOpts(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("hydrophobic_dist", "hbond_dist", "hbond_angle", "ionic_dist", "cation_pi_dist",
                                         "cation_pi_offset", "pi_dist", "pi_offset", "face_angle", "edge_angle", "xbond_dist",
                                         "xbond_donor_angle", "xbond_acceptor_min", "xbond_acceptor_max")]


class InteractionsOut(C.Structure):
    _fields_ = [("bits", C.c_void_p), ("counts", C.c_void_p)]


class PocketCheckIn(C.Structure):
    _fields_ = [("n_group", C.c_int32), ("n_frame", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("frame_ptr", "pocket_ptr", "pocket_pos_off", "pocket_pos", "pocket_rad", "pocket_col",
                                          "pocket_rank", "static_ptr", "static_pos", "static_rad", "static_col", "mov_ptr", "mov_atom",
                                          "excl_ptr", "excl", "closure_ptr", "closure_ab", "closure_len", "res_ptr", "res_off")] + \
               [(n, C.c_int32) for n in ("max_pocket", "max_excl", "max_res", "cand_cap")] + [("host", C.c_void_p)]


class PocketCheckOpts(C.Structure):
    _fields_ = [("clash_ratio", C.c_float), ("bond_tol", C.c_float), ("max_clashes", C.c_int32)]


class PocketCheckOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("n_clash", "min_ratio", "worst_pair", "res_clash", "n_broken", "max_bond_dev", "passed")]


class SasaIn(C.Structure):
    _fields_ = [("n_group", C.c_int32), ("n_frame", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("frame_ptr", "lig_ptr", "lig_pos_off", "lig_pos", "lig_rad", "lig_w", "lig_polar", "pocket_ptr",
                                          "pocket_pos_off", "pocket_pos", "pocket_rad", "pocket_w", "pocket_col", "pocket_polar",
                                          "static_ptr", "static_pos", "static_rad", "static_w", "static_col", "static_polar", "res_ptr",
                                          "res_off", "points")] + \
               [(n, C.c_int32) for n in ("n_points", "max_lig", "max_pocket", "max_res", "cand_cap")] + [("host", C.c_void_p)]


class SasaOpts(C.Structure):
    _fields_ = [("probe", C.c_float)]


class SasaOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("lig_free", "lig_bound", "res_buried", "totals")]


class CavityIn(C.Structure):
    _fields_ = [("n_group", C.c_int32), ("n_frame", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("frame_ptr", "lig_ptr", "lig_pos_off", "lig_pos", "lig_rad", "pocket_ptr", "pocket_pos_off",
                                          "pocket_pos", "pocket_rad", "pocket_col", "pocket_polar", "static_ptr", "static_pos",
                                          "static_rad", "static_col", "static_polar", "res_ptr", "res_off", "grid_lo", "ref_frame")] + \
               [(n, C.c_int32) for n in ("max_lig", "max_pocket", "max_res")] + [("host", C.c_void_p)]


class CavityOpts(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("spacing", "probe", "ray_length", "lining_cutoff")] + [("min_buried", C.c_int32)]


class CavityOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("totals", "lining", "masks", "burial", "workspace")] + [("workspace_bytes", C.c_size_t)]


class HoloSiteIn(C.Structure):
    _fields_ = [("n_pair", C.c_int32)] + [(n, C.c_void_p) for n in ("atom_ptr", "atom_pos", "atom_res", "lig_ptr", "lig_pos", "res_ptr")] + \
               [("n_res", C.c_int32), ("max_atoms", C.c_int32), ("cutoff", C.c_float)]


class HoloMetricsIn(C.Structure):
    _fields_ = [("n_group", C.c_int32), ("n_frame", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("frame_ptr", "site_ptr", "site_aatype", "site_row", "site_matched", "holo14", "holo_mask", "apo14",
                                          "frame_mask", "holo_chi", "site_off", "res_ptr", "pocket_off", "pocket", "hlig_ptr", "hlig",
                                          "pair_off", "lig_ptr", "lig_off", "lig", "perm_ptr", "perm_off", "perms")] + \
               [(n, C.c_int32) for n in ("max_site", "max_res", "max_lig")] + [("host", C.c_void_p)]


class HoloMetricsOpts(C.Structure):
    _fields_ = [("radius", C.c_float)]


class HoloMetricsOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("pair_dist", "plddt_den", "lddt_den", "sc_rmsd", "sc_sq_sum", "sc_n", "chi", "altchi", "dchi",
                                          "plddt_num", "lddt_num")]


class HeteroCheckIn(C.Structure):
    _fields_ = [("n_group", C.c_int32), ("n_frame", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("frame_ptr", "lig_ptr", "lig_pos_off", "lig_pos", "lig_rad", "lig_cov", "lig_flags", "het_ptr",
                                          "het_pos", "het_rad", "het_cov", "het_class", "het_metal", "pocket_ptr", "pocket_pos_off",
                                          "pocket_pos", "pocket_polar", "pocket_col", "static_ptr", "static_pos", "static_polar",
                                          "static_col", "res_ptr")] + \
               [(n, C.c_int32) for n in ("max_lig", "max_pocket", "max_res", "cand_cap")] + [("host", C.c_void_p)]


class HeteroCheckOpts(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("clash_ratio", "displace_dist", "metal_dist", "hbond_dist", "grid")] + \
               [("vol_scale", C.c_float * 3), ("vol_overlap_max", C.c_float * 3), ("max_event", C.c_int32)]


class HeteroCheckOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("min_dist", "min_ratio", "worst", "n_clash", "vol_lig", "vol_overlap", "n_displaced", "n_bridge",
                                          "n_coord", "passed", "event_i", "event_f", "n_event")]


class HydrogensIn(C.Structure):
    _fields_ = [("n_group", C.c_int32), ("n_frame", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("frame_ptr", "lig_ptr", "lig_pos_off", "lig_pos", "lig_acc", "lig_nbr", "lh_ptr", "lh_i", "lh_f",
                                          "lrot_ptr", "lrot_i", "lrot_f", "lh_out_off", "lk_off", "pocket_ptr", "pocket_pos_off",
                                          "pocket_pos", "pocket_meta", "static_ptr", "static_pos", "static_meta", "rh_ptr", "rh_i", "rh_f",
                                          "rrot_ptr", "rrot_i", "rrot_f", "rh_out_off", "rk_off", "res_ptr", "res_off")] + \
               [(n, C.c_int32) for n in ("max_lig", "max_lig_h", "max_lig_rot", "max_rec_h", "max_res", "cand_cap")] + [("host", C.c_void_p)]


class HydrogensOpts(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("hb_dist", "hb_h_dist", "hb_dha_angle", "hb_acc_angle")] + [("max_bond", C.c_int32)]


class HydrogensOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("lig_h", "rec_h", "lig_k", "rec_k", "counts", "n_bond", "bond_i", "bond_f", "res_bits")]


class VinaDecomposeIn(C.Structure):
    _fields_ = [("n_group", C.c_int32), ("n_frame", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("frame_ptr", "lig_ptr", "lig_pos_off", "lig_pos", "lig_type", "pocket_ptr", "pocket_pos_off",
                                          "pocket_pos", "pocket_type", "pocket_col", "static_ptr", "static_pos", "static_type",
                                          "static_col", "col_ptr", "col_off")] + \
               [(n, C.c_int32) for n in ("max_lig", "max_col")] + [("host", C.c_void_p)]


class VinaDecomposeOpts(C.Structure):
    _fields_ = [("cutoff", C.c_float)]


class VinaDecomposeOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("col_terms", "atom_terms", "totals", "col_fixed", "atom_fixed", "totals_fixed")]


class PocketStatesIn(C.Structure):
    _fields_ = [("n_group", C.c_int32), ("n_frame", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("frame_ptr", "res_ptr", "pocket_off", "pocket", "aatype", "atom14_mask", "res_mask", "ref_last",
                                          "pair_off")] + \
               [("max_frame", C.c_int32), ("max_res", C.c_int32), ("host", C.c_void_p)]


class PocketStatesOpts(C.Structure):
    _fields_ = [("ref_last", C.c_int32), ("tile_rows", C.c_int32)]


class PocketStatesOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("dist_max", "dist_pooled", "worst_res", "chi", "rot", "n_rot", "top_rot", "top_count", "ref_rot",
                                          "ref_count", "mob_max", "mob_sq", "dev_ref_max", "n_used", "frame_ok")]


class ShapeIn(C.Structure):
    _fields_ = [("n_mol", C.c_int32), ("n_cloud", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("mol_atom_ptr", "alpha", "flags", "color_alpha", "mol_grp_ptr", "grp", "cloud_mol", "cloud_pos_off",
                                          "pos", "a_ptr", "a_cloud", "b_ptr", "b_cloud", "pair_off")] + \
               [("n_set", C.c_int32), ("max_a", C.c_int32), ("max_b", C.c_int32), ("n_pos_row", C.c_int64), ("host", C.c_void_p)]


class ShapeOpts(C.Structure):
    _fields_ = [("color_weight", C.c_float), ("b_tile", C.c_int32)]


class ShapeOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("self_fixed", "pair_fixed", "tanimoto", "dist")]


class PdbLigand(C.Structure):
    _fields_ = [("n_atoms", i32), ("head", C.c_char_p), ("atom_line", C.POINTER(C.c_char_p)), ("tail", C.c_char_p)]


class XtcIn(C.Structure):
    _fields_ = [(n, i32) for n in ("n_frame", "n_file", "n_src", "n_lig", "n_res", "n_static", "n_map", "max_atoms")] + \
               [(n, vp) for n in ("lig", "pos14", "center", "static_pos", "map_ptr", "atom_map", "file_map", "frame_file",
                                  "frame_src", "frame_step")]


class XtcOpts(C.Structure):
    _fields_ = [("precision", f32), ("dt", f32), ("first_step", i32), ("box", f32 * 9)]


class SitesOpts(C.Structure):
    _fields_ = [(n, f32) for n in ("spacing", "probe", "ray_length", "lining_cutoff")] + \
               [(n, i32) for n in ("min_buried", "min_points", "max_sites")]


class SitesIn(C.Structure):
    _fields_ = [("n_prot", i32), ("n_res", i32), ("max_points", C.c_int64)] + \
               [(n, vp) for n in ("res_ptr", "aatype", "atom37_pos", "atom37_mask", "radius")]


class SitesOut(C.Structure):
    _fields_ = [(n, vp) for n in ("n_sites", "label", "n_points", "score", "idx_sum", "centre", "lining", "grid", "occupancy",
                                  "burial", "labels")]


# every typedef struct of include/dbfr.h -> its mirror above (tests/test_abi_host.py compares names, order, kinds, sizes and offsets)
STRUCTS = {
    "dbfr_model_cfg": ModelCfg, "dbfr_tensor": Tensor, "dbfr_batch": Batch, "dbfr_limits": Limits, "dbfr_cond": Cond,
    "dbfr_scores": Scores, "dbfr_step": Step, "dbfr_noise": Noise, "dbfr_init_tape": InitTape,
    "dbfr_pose_metrics_in": PoseMetricsIn, "dbfr_pose_metrics_out": PoseMetricsOut, "dbfr_pdb_topology": PdbTopology,
    "dbfr_pdb_ligand": PdbLigand, "dbfr_sdf_template": SdfTemplate, "dbfr_mdn_batch": MdnBatch, "dbfr_mdn_seg": MdnSeg, "dbfr_mdn_vseg": MdnVSeg,
    "dbfr_vina_in": VinaIn, "dbfr_vina_opts": VinaOpts, "dbfr_vina_search_opts": VinaSearchOpts, "dbfr_vina_flex_in": VinaFlexIn,
    "dbfr_pose_rmsd_in": PoseRmsdIn, "dbfr_modes_opts": ModesOpts,
    "dbfr_pose_check_in": PoseCheckIn, "dbfr_pose_check_opts": PoseCheckOpts, "dbfr_pose_check_out": PoseCheckOut,
    "dbfr_interactions_in": InteractionsIn, "dbfr_interactions_opts": InteractionsOpts, "dbfr_interactions_out": InteractionsOut,
    "dbfr_pocket_check_in": PocketCheckIn, "dbfr_pocket_check_opts": PocketCheckOpts, "dbfr_pocket_check_out": PocketCheckOut,
    "dbfr_sasa_in": SasaIn, "dbfr_sasa_opts": SasaOpts, "dbfr_sasa_out": SasaOut,
    "dbfr_cavity_in": CavityIn, "dbfr_cavity_opts": CavityOpts, "dbfr_cavity_out": CavityOut,
    "dbfr_holo_site_in": HoloSiteIn, "dbfr_holo_metrics_in": HoloMetricsIn, "dbfr_holo_metrics_opts": HoloMetricsOpts,
    "dbfr_holo_metrics_out": HoloMetricsOut,
    "dbfr_hetero_check_in": HeteroCheckIn, "dbfr_hetero_check_opts": HeteroCheckOpts, "dbfr_hetero_check_out": HeteroCheckOut,
    "dbfr_hydrogens_in": HydrogensIn, "dbfr_hydrogens_opts": HydrogensOpts, "dbfr_hydrogens_out": HydrogensOut,
    "dbfr_vina_decompose_in": VinaDecomposeIn, "dbfr_vina_decompose_opts": VinaDecomposeOpts,
    "dbfr_vina_decompose_out": VinaDecomposeOut,
    "dbfr_pocket_states_in": PocketStatesIn, "dbfr_pocket_states_opts": PocketStatesOpts, "dbfr_pocket_states_out": PocketStatesOut,
    "dbfr_shape_in": ShapeIn, "dbfr_shape_opts": ShapeOpts, "dbfr_shape_out": ShapeOut,
    "dbfr_xtc_in": XtcIn, "dbfr_xtc_opts": XtcOpts, "dbfr_sites_opts": SitesOpts, "dbfr_sites_in": SitesIn, "dbfr_sites_out": SitesOut,
}

P, i64, u64, f64, sz, cp = C.POINTER, C.c_int64, C.c_uint64, C.c_double, C.c_size_t, C.c_char_p
_TEST_CONV = [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp]

# every function of include/dbfr.h -> its argtypes (the same test compares arity, scalar kinds and struct-pointer targets)
PROTOTYPES = {
    "dbfr_abi_version": [],
    "dbfr_build_id": [],
    "dbfr_last_error": [],
    "dbfr_model_create": [P(ModelCfg), P(Tensor), i32, P(vp)],
    "dbfr_model_destroy": [vp],
    "dbfr_model_set_edge_log": [vp, vp, i32, i32],
    "dbfr_model_set_tie_log": [vp, vp, i32, i32, f32],
    "dbfr_model_fallback_convs": [vp, cp, sz],
    "dbfr_model_rowscaled_convs": [vp, cp, sz],
    "dbfr_model_set_gemm": [vp, i32],
    "dbfr_model_get_gemm": [vp],
    "dbfr_workspace_bytes": [vp, P(Batch), P(Limits), P(sz)],
    "dbfr_score": [vp, P(Batch), P(Cond), P(Scores), vp, sz, P(Limits), vp],
    "dbfr_sample": [vp, P(Batch), P(Step), i32, P(Noise), vp, vp, vp, vp, sz, P(Limits), vp],
    "dbfr_sample_range": [vp, P(Batch), P(Step), i32, i32, P(Noise), vp, vp, vp, vp, sz, P(Limits), vp],
    "dbfr_capacity_report": [vp, vp, P(i32), P(i64)],
    "dbfr_init_poses": [vp, P(Batch), P(InitTape), vp, vp],
    "dbfr_extract_templates": [i32, vp, vp, vp, vp, vp, vp, vp, vp],
    "dbfr_status_sync": [vp, vp, P(i64)],
    "dbfr_wigner3j": [i32, i32, i32, P(f64)],
    "dbfr_conv_paths": [i32, P(i32), i32, P(i32)],
    "dbfr_test_pack_f16_tiles": [vp, vp, i32, vp, P(i32)],
    "dbfr_test_pack_f16_depth": [vp, vp, i32, P(i32), P(i32)],
    "dbfr_test_pack_f16_rows": [vp, vp, i32, vp, P(i32), vp, P(i32)],
    "dbfr_test_pack_conv": [i32, vp, i32, vp, vp, i32, cp, sz, P(i32)],
    "dbfr_test_chunk_table": [vp, vp, i32, i32, vp, i32, vp, vp, vp],
    "dbfr_probe_mfma_f16": [f64, P(f64), vp],
    "dbfr_profile_enable": [vp, i32],
    "dbfr_profile_fused_bytes": [vp, P(f64)],
    "dbfr_profile_executed_flops": [vp, P(f64)],
    "dbfr_profile_useful_flops": [vp, P(f64), P(f64)],
    "dbfr_profile_read": [vp, P(f64), P(i64), P(f64), P(f64), i32],
    "dbfr_workspace_layout": [vp, P(Batch), P(Limits), cp, sz, P(sz), P(sz), i32],
    "dbfr_test_conv": _TEST_CONV,
    "dbfr_test_conv2": _TEST_CONV,
    "dbfr_test_reduce_ln": [vp, i32, i32, vp, vp, vp, i32, vp, i32, vp, i32, vp],
    "dbfr_test_reduce_ln2": [vp, i32, i32, vp, vp, vp, i32, vp, i32, vp, i32, vp, vp],
    "dbfr_test_sde_step": [vp, P(Batch), P(Step), P(Scores), P(Noise), vp, vp, vp],
    "dbfr_test_time_embed": [vp, vp, i32, vp, vp],
    "dbfr_test_mlp": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "dbfr_test_atom_encoder": [vp, vp, vp, vp, i32, vp, vp],
    "dbfr_test_reduce_ln_layer": [vp, i32, P(vp), P(vp), P(vp), P(vp), i32, i32, vp, vp, vp, vp, vp],
    "dbfr_test_center_edges": [P(Batch), vp, vp, vp, vp, vp, vp, vp],
    "dbfr_test_trrot": [vp, vp, vp, vp, vp, i32, vp, vp, vp, vp],
    "dbfr_test_bond_attr": [vp, i32, vp, i32, vp, vp, vp, i32, vp, vp],
    "dbfr_test_tor_final": [vp, i32, vp, vp, i32, vp, vp],
    "dbfr_select_pocket": [i32, i32, vp, i32, vp, vp, vp, vp, f64, i32, vp, vp, vp],
    "dbfr_pose_metrics": [P(PoseMetricsIn), P(PoseMetricsOut), vp],
    "dbfr_pdb_format": [P(PdbTopology), i32, vp, vp, i32, i32, vp, i64],
    "dbfr_pdb_write_files": [P(PdbTopology), i32, vp, vp, i32, P(cp), i32],
    "dbfr_sdf_format": [P(SdfTemplate), vp, vp, i64],
    "dbfr_sdf_write_files": [P(SdfTemplate), vp, i32, P(cp), i32],
    "dbfr_mdn_model_create": [P(Tensor), i32, P(vp)],
    "dbfr_mdn_model_destroy": [vp],
    "dbfr_mdn_workspace_bytes": [P(MdnBatch), P(sz)],
    "dbfr_mdn_pocket_features": [i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp],
    "dbfr_mdn_forward": [vp, P(MdnBatch), vp, vp, vp, vp, sz, vp],
    "dbfr_test_mdn_lin": [P(MdnSeg), i32, vp, i32, vp, i32, i32, i32, vp, i32, i32, vp, i32, vp],
    "dbfr_test_mdn_gt_attn": [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp],
    "dbfr_test_mdn_gvp": [P(MdnVSeg), i32, P(MdnSeg), i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp],
    "dbfr_test_mdn_gvp_ln": [vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp],
    "dbfr_test_mdn_mean_in": [vp, i32, vp, i32, vp, i32, vp, vp, vp],
    "dbfr_test_mdn_seq_concat": [vp, vp, vp, i32, vp, vp],
    "dbfr_test_mdn_gt_layer": [vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, sz, vp],
    "dbfr_test_mdn_head": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, vp, vp, sz, vp],
    "dbfr_vina_workspace_bytes": [P(VinaIn), P(sz)],
    "dbfr_vina_score": [P(VinaIn), vp, vp, vp, vp, sz, vp],
    "dbfr_vina_score_at": [P(VinaIn), vp, vp, vp, vp, vp, vp, vp, sz, vp],
    "dbfr_vina_minimize": [P(VinaIn), P(VinaOpts), vp, vp, vp, vp, sz, vp],
    "dbfr_vina_flex_workspace_bytes": [P(VinaFlexIn), P(sz)],
    "dbfr_vina_flex_score_at": [P(VinaFlexIn), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp],
    "dbfr_vina_flex_minimize": [P(VinaFlexIn), P(VinaOpts), vp, vp, vp, vp, vp, vp, sz, vp],
    "dbfr_vina_search_workspace_bytes": [P(VinaIn), i32, P(sz)],
    "dbfr_vina_search": [P(VinaIn), P(VinaOpts), P(VinaSearchOpts), vp, vp, vp, vp, vp, vp, vp, vp, sz, vp],
    "dbfr_vina_flex_search_workspace_bytes": [P(VinaFlexIn), i32, P(sz)],
    "dbfr_vina_flex_search": [P(VinaFlexIn), P(VinaOpts), P(VinaSearchOpts), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp],
    "dbfr_test_philox4x32": [P(C.c_uint32), P(C.c_uint32), P(C.c_uint32)],
    "dbfr_test_vina_mutation": [u64, i64, i32, i32, i32, f32, f32, P(i32), P(f32)],
    "dbfr_pose_rmsd_matrix": [P(PoseRmsdIn), vp, vp],
    "dbfr_select_modes": [P(PoseRmsdIn), vp, vp, P(ModesOpts), vp, vp, vp, vp],
    "dbfr_pose_check": [P(PoseCheckIn), P(PoseCheckOpts), P(PoseCheckOut), vp],
    "dbfr_pdb_atom_map": [P(PdbTopology), i32, vp, vp, vp, i64, P(i64)],
    "dbfr_complex_pdb_format": [P(PdbTopology), i32, vp, vp, P(PdbLigand), vp, vp, i64],
    "dbfr_complex_pdb_write_files": [P(PdbTopology), i32, vp, vp, P(PdbLigand), vp, i32, P(cp), i32],
    "dbfr_xtc_workspace_bytes": [P(XtcIn), P(sz), P(i64)],
    "dbfr_xtc_encode": [P(XtcIn), P(XtcOpts), vp, i64, vp, vp, sz, vp],
    "dbfr_sites_workspace_bytes": [P(SitesIn), P(sz)],
    "dbfr_find_sites": [P(SitesIn), P(SitesOpts), P(SitesOut), vp, sz, vp],
    "dbfr_interactions": [P(InteractionsIn), P(InteractionsOpts), P(InteractionsOut), vp],
    "dbfr_pocket_check": [P(PocketCheckIn), P(PocketCheckOpts), P(PocketCheckOut), vp],
    "dbfr_sasa": [P(SasaIn), P(SasaOpts), P(SasaOut), vp],
    "dbfr_seq_align": [i32, vp, vp, vp, vp, vp, vp, i32],
    "dbfr_holo_site": [P(HoloSiteIn), vp, vp],
    "dbfr_holo_metrics": [P(HoloMetricsIn), P(HoloMetricsOpts), P(HoloMetricsOut), vp],
    "dbfr_hetero_check": [P(HeteroCheckIn), P(HeteroCheckOpts), P(HeteroCheckOut), vp],
    "dbfr_hydrogens": [P(HydrogensIn), P(HydrogensOpts), P(HydrogensOut), vp],
    "dbfr_vina_decompose": [P(VinaDecomposeIn), P(VinaDecomposeOpts), P(VinaDecomposeOut), vp],
    "dbfr_pose_cavity_workspace_bytes": [P(CavityIn), P(sz)],
    "dbfr_pose_cavity": [P(CavityIn), P(CavityOpts), P(CavityOut), vp],
    "dbfr_pocket_states": [P(PocketStatesIn), P(PocketStatesOpts), P(PocketStatesOut), vp],
    "dbfr_shape_overlap": [P(ShapeIn), P(ShapeOpts), P(ShapeOut), vp],
}
# the return types that are not int
RESTYPES = {"dbfr_last_error": cp, "dbfr_build_id": cp, "dbfr_model_destroy": None, "dbfr_mdn_model_destroy": None,
            "dbfr_pdb_format": i64, "dbfr_sdf_format": i64, "dbfr_pdb_atom_map": i64, "dbfr_complex_pdb_format": i64}
SYMBOLS = list(PROTOTYPES)
ABI_VERSION = 9                 # DBFR_ABI_VERSION


@lru_cache(maxsize=None)
def pointer_fields(cls, skip=2):
    """The run of pointer (c_void_p) fields behind the first `skip` fields of a struct: the arrays of an input struct, between its
    leading counts (or VinaFlexIn's `base`, skip=1) and its trailing ints."""
    return [f for f, _ in takewhile(lambda f: f[1] is C.c_void_p, cls._fields_[skip:])]


_lib = None


class DbfrError(RuntimeError):
    pass


def load():
    """Load libdbfr.so; raises if it has not been built (python -m diffbindfr_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DbfrError(f"{LIB_PATH} is missing: build the HIP library first "
                        f"(python -m diffbindfr_amd.build). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        if name in RESTYPES:
            fn.restype = RESTYPES[name]
    if lib.dbfr_abi_version() != ABI_VERSION:
        raise DbfrError("libdbfr ABI version mismatch")
    _lib = lib
    return lib


def check(rc):
    if rc != DBFR_OK:
        msg = load().dbfr_last_error().decode()
        raise DbfrError(f"{ERRORS.get(rc, rc)}: {msg}")


def workspace_views(model_handle, batch_c, limits, ws):
    """dict name -> uint8 view of the internal buffer inside the torch workspace (tests/debug)."""
    lib = load()
    names = C.create_string_buffer(8192)
    offs = (C.c_size_t * 128)()
    nbytes = (C.c_size_t * 128)()
    n = lib.dbfr_workspace_layout(model_handle, C.byref(batch_c), C.byref(limits), names, 8192, offs, nbytes, 128)
    if n < 0:
        check(n)
    out = {}
    for i, nm in enumerate(names.value.decode().split(";")[:n]):
        out[nm] = ws[offs[i]:offs[i] + nbytes[i]]
    return out
