"""The Vina stage is split over vina_typing / vina_batch / vina_flex / vina_entries; ``vina`` re-exports all of it.  The names that
tests, tools and other modules reach as ``vina.<name>`` stay reachable, typing loads without the device classes, and the search's
best-chain pick is checked on CPU tensors."""
import torch

from diffbindfr_amd import vina

NAMES = """XS XS_NAMES DUMMY MET_D BOND_TOLERANCE TERMS FLEX_TERMS MAX_TORSIONS FLEX_MAX_SLOTS FLEX_MAX_VARS FLEX_MAX_EXCL FLEX_COLUMNS
SEARCH_DEFAULTS SEARCH_LOG SEARCH_COLUMNS
parse_molblock ligand_types hetero_bonds hetero_types receptor_type_table pocket_types intra_pairs _tables
VinaBatch VinaFlexBatch PoseBatch score_poses minimize_poses search_poses
residue_flex_sets flex_topology select_flexible _flex_sets
_entry_receptor _entry_arrays _entry_batch refine_entry refine_entry_flex search_entry search_entry_flex refined_entry error_correct
DbfrError""".split()


def test_vina_reexports_every_public_name():
    missing = [n for n in NAMES if not hasattr(vina, n)]
    assert not missing, missing
    assert vina.__doc__ and "Specification" in vina.__doc__


def test_typing_module_does_not_define_the_device_classes():
    from diffbindfr_amd import vina_typing
    assert vina.ligand_types is vina_typing.ligand_types and vina.XS is vina_typing.XS
    assert not hasattr(vina_typing, "VinaBatch") and not hasattr(vina_typing, "error_correct")


def test_best_chain_pick():
    nan, inf = float("nan"), float("inf")
    obj = torch.tensor([[3.0, nan, 1.0, nan, 2.0],       # chain 0
                        [1.0, 5.0, 1.0, nan, nan],       # chain 1
                        [1.0, 4.0, 2.0, nan, 2.0]])      # chain 2
    terms = torch.zeros(3, 5, 8)
    terms[:, :, 6] = obj
    pick = vina._best_chain(terms)
    assert pick.dtype == torch.int64 and pick.shape == (5,)
    # lowest objective; a tie goes to the lowest chain; NaN counts as +inf (so it loses to a number and ties with NaN)
    assert pick[:3].tolist() == [1, 2, 0] and pick[4].item() == 0
    assert 0 <= pick[3].item() < 3                     # an all-NaN column still picks a chain that exists
    terms[:, :, 6] = torch.tensor([[inf], [nan], [inf]]).expand(3, 5)
    assert vina._best_chain(terms).tolist() == [0] * 5
    assert vina._best_chain(terms[:1]).tolist() == [0] * 5
