"""Time-varying AMR volumes without a device: the designed fields of tests/volume_amr_update_cases.py do what they claim (by the numpy
checker alone, so a merge that forgets the subgrids cannot pass the GPU test), and the comparison of subgrid trees that
HipVolumeAdapter.update_amr and VolumeTracer.update(amr=True) run before anything changes."""
from types import SimpleNamespace

import numpy as np
import pytest

from gravit_amd import scenes
from gravit_amd.adapter import same_subgrid_tree, subgrid_tree
from gravit_amd.scheduler import VolumeTracer
from tests import volume_amr_cases as cases
from tests import volume_amr_checker as ac
from tests import volume_amr_update_cases as uc
from tests.volume_common import IDENT

F = np.float32


def empty(vol, subgrids=None):
    B = ac.AmrBrick(vol, uc.half(), uc.RATE, subgrids)
    return ac.empty_blocks(B, *ac.ranges(B))


@pytest.mark.parametrize("which", sorted(uc.DESIGNED))
def test_only_the_subgrids_new_samples_open_the_target_cells(which):
    a, b = uc.designed(which)
    cells = uc.DESIGNED[which]["cells"]
    ea, eb = empty(a), empty(b)
    assert ea.all() and ea.size == 27
    assert not any(eb[c] for c in cells) and eb.sum() == 27 - len(cells)
    assert (a.data == b.data).all()  # level 0 is the same array: the subgrid alone makes the difference ...
    assert empty(b, subgrids=[]).all() and empty(a, subgrids=[]).all()  # ... and the brick without subgrids is empty in both steps
    # ... and the GPU test's aimed rays see it: opacity in B, none in A
    d = uc.DESIGNED[which]
    aimed = uc.aimed_rays(a, uc.vertex_position(a, d["subgrid"], d["vertex"]))
    assert (ac.march(ac.AmrBrick(b, uc.half(), uc.RATE), aimed, IDENT)["w"] > 0).sum() > 8
    assert not (ac.march(ac.AmrBrick(a, uc.half(), uc.RATE), aimed, IDENT)["w"] > 0).any()
    if which == "boundary":  # the vertex lies ON the level-0 plane x = 8, strictly inside one macro cell on y and z
        p = uc.vertex_position(b, d["subgrid"], d["vertex"])
        g = (p - np.asarray(b.origin, np.float64)) / np.asarray(b.spacing, np.float64)
        assert abs(g[0] - 8.0) < 1e-9 and 0 < g[1] < 8 and 0 < g[2] < 8 and g[1] % 1 and g[2] % 1


def test_the_steps_share_a_tree_and_differ_everywhere():
    a, b = uc.step(0), uc.step(1)
    assert subgrid_tree(a.subgrids) == subgrid_tree(b.subgrids) and len(a.subgrids) == 4
    assert (a.data != b.data).mean() > 0.9 and all((s.data != t.data).mean() > 0.9 for s, t in zip(a.subgrids, b.subgrids))
    for kind in uc.NONFINITE:
        s0 = uc.nonfinite(kind).subgrids[0].data
        assert np.isnan(s0).any() == (kind != "inf") and np.isinf(s0).any() == (kind != "nan")
        _, _, wild = ac.ranges(ac.AmrBrick(uc.nonfinite(kind), uc.half(), uc.RATE))
        assert wild.any() and not ac.ranges(ac.AmrBrick(b, uc.half(), uc.RATE))[2].any()


def test_the_tree_comparison_accepts_an_equal_tree_and_names_what_changed():
    vol = uc.step(0)
    tree = subgrid_tree(vol.subgrids)
    assert tree[1] == (0, 4, cases.S1["lo"], cases.S1["cells"]) and subgrid_tree(None) == [] and subgrid_tree([]) == []
    same_subgrid_tree(tree, vol.subgrids)
    same_subgrid_tree(tree, uc.step(1).subgrids)  # other data, the same tree
    same_subgrid_tree([], None)
    for what, subs in uc.changed_trees(vol).items():
        with pytest.raises(ValueError, match="given" if what == "count" else what.split()[0]):
            same_subgrid_tree(tree, subs)
    with pytest.raises(ValueError):
        same_subgrid_tree(tree, [])
    with pytest.raises(ValueError):
        same_subgrid_tree([], vol.subgrids)


def test_update_with_amr_checks_every_tree_before_the_first_brick_changes():
    parts = scenes.split_amr_volume(uc.step(0), 2, 2, 2, cuts=cases.CUTS)
    nxt = scenes.split_amr_volume(uc.step(1), 2, 2, 2, cuts=cases.CUTS)
    pushed = []
    ads = [SimpleNamespace(counts=b.counts, offset=b.offset, tree=subgrid_tree(b.subgrids), update_samples=lambda d, i=i: pushed.append(("plain", i)),
                           update_amr=lambda d, s, i=i: pushed.append(("amr", i, len(s)))) for i, b in enumerate(parts)]
    tr = SimpleNamespace(adapters=ads, _same_bricking=VolumeTracer._same_bricking)
    assert VolumeTracer.update(tr, nxt, amr=True) is tr and tr._grid_stale
    holders = [i for i, b in enumerate(parts) if b.subgrids]
    assert len(holders) >= 2 and pushed == [("amr", i, len(parts[i].subgrids)) if i in holders else ("plain", i) for i in range(8)]
    del pushed[:]
    last = holders[-1]
    for what, subs in uc.changed_trees(nxt[holders[0]]).items():
        bad = list(nxt)
        bad[holders[0]] = scenes.Brick(**{**nxt[holders[0]].__dict__, "subgrids": subs})
        with pytest.raises(ValueError, match="brick %d" % holders[0]):
            VolumeTracer.update(tr, bad, amr=True)
    bad = list(nxt)
    bad[last] = scenes.Brick(**{**nxt[last].__dict__, "subgrids": []})  # the LAST brick with subgrids lost them: nothing before it may change
    with pytest.raises(ValueError, match="brick %d" % last):
        VolumeTracer.update(tr, bad, amr=True)
    assert pushed == []
    # without the keyword nothing is compared and every brick takes update_samples, as ever
    assert VolumeTracer.update(tr, bad) is tr and pushed == [("plain", i) for i in range(8)]
