"""nbdt_group_logits, nbdt_group_logits_backward, nbdt_superclass_accumulate and the analyzers of nbdt.superclass on the
MI355X against the numpy restatement tests/_superclass_ref.py.  Every comparison is exact: bit-equal floats (compared as
their uint32 patterns, so NaN columns compare too), equal integers.  Where torch's own mean / autograd is the yardstick
the fixtures make every sum exactly representable (integer logits below 2^10, power-of-two group sizes, integer
gradients), so the order of a sum cannot matter."""
from collections import defaultdict

import numpy as np
import pytest
import torch

import _superclass_ref as R

pytestmark = pytest.mark.gpu

from nbdt import _C  # noqa: E402
from nbdt import superclass as S  # noqa: E402
from nbdt.model import EmbeddedDecisionRules  # noqa: E402
from nbdt.tree import Tree  # noqa: E402

DEV = "cuda:0"
MODES = (R.MASKED, R.GROUP_MEAN)
CIFAR_MAP = [1, -1, 0, 0, 0, 0, 0, 0, 1, -1]          # animal / vehicle over CIFAR10 from the shipped graph
CIFAR_GROUPS = [[2, 3, 4, 5, 6, 7], [0, 8]]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def same_bits(got, want):
    return np.array_equal(bits(got), bits(want))


def map_of(groups, C):
    m = [-1] * C
    for g, members in enumerate(groups):
        for c in members:
            if m[c] < 0:
                m[c] = g
    return m


def dev_i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def accumulate(groups, C, z, y, map_target, map_pred, mode, totals=None, confusion=None):
    """One launch through the binding: (totals, confusion [G, G], pred) as numpy.  z: a tensor (any supported layout)."""
    G = len(groups)
    handle = _C.groups_handle(groups, C, 0)
    totals = torch.zeros(2, dtype=torch.int64, device=DEV) if totals is None else totals
    confusion = torch.zeros(G * G, dtype=torch.int64, device=DEV) if confusion is None else confusion
    pred = _C.superclass_accumulate(handle, z.to(DEV), torch.as_tensor(y, dtype=torch.int64).to(DEV), dev_i32(map_target),
                                    dev_i32(map_pred), mode, totals, confusion, want_pred=True)
    return totals.cpu().numpy(), confusion.cpu().numpy().reshape(G, G), pred.cpu().numpy()


def check_both_modes(groups, C, z, y, map_target, map_pred, z_ref=None):
    z_ref = z.float().cpu().numpy() if z_ref is None else z_ref
    for mode in MODES:
        got = accumulate(groups, C, z, y, map_target, map_pred, mode)
        want = R.accumulate(z_ref, y, map_target, map_pred, groups, mode)
        for g, w, what in zip(got, want, ("totals", "confusion", "pred")):
            assert np.array_equal(g, w), (mode, what, g, w)
    got = _C.group_logits(_C.groups_handle(groups, C, 0), z.to(DEV)).cpu().numpy()
    assert same_bits(got, R.group_logits(z_ref, groups))


# ------------------------------------------------------------------------------------------------ shapes and types
@pytest.fixture(scope="module")
def small():
    """300 rows of C = 10 logits, labels over C_test = 200 (a few invalid), a random test mapping.  Read-only."""
    rng = np.random.default_rng(11)
    z = (rng.standard_normal((300, 16)) * 3).astype(np.float32)
    y = rng.integers(0, 200, 300)
    y[[5, 70]] = [-1, 200]
    map_target = rng.integers(-1, 2, 200).tolist()
    return z, y, map_target


@pytest.mark.parametrize("pad", [0, 6])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 64, 65, 100])
def test_both_modes_on_the_cifar10_grouping(small, B, dtype, pad):
    z16, y, map_target = small
    z = torch.from_numpy(z16[:B, :10 + pad].copy()).to(dtype).to(DEV)[:, :10]   # a view on the device: ldz = 10 or 16
    assert z.stride(0) == 10 + pad and z.is_cuda
    z_ref = R.bf16_round(z16[:B, :10]) if dtype == torch.bfloat16 else z16[:B, :10]
    check_both_modes(CIFAR_GROUPS, 10, z, y[:B], map_target, CIFAR_MAP, z_ref)
    totals = R.accumulate(z_ref, y[:B], map_target, CIFAR_MAP, CIFAR_GROUPS, R.MASKED)[0]
    assert B == 1 or 0 < totals[1] < totals[0] < B                               # the fixture exercises every counter


def scattered_groups(C, sizes, seed):
    order = np.random.default_rng(seed).permutation(C).tolist()          # members in no particular order: the LISTED one
    groups, at = [], 0
    for n in sizes:
        groups.append(order[at:at + n])
        at += n
    return groups


def test_uneven_groups():
    C, B = 1000, 33
    groups = scattered_groups(C, (1, 2, 397, 64, 3), 2)
    rng = np.random.default_rng(3)
    z = (rng.standard_normal((B, C)) * 2).astype(np.float32)
    y = rng.integers(0, C, B)
    map_pred = map_of(groups, C)
    assert map_pred.count(-1) == 1000 - 467
    check_both_modes(groups, C, torch.from_numpy(z), y, map_pred, map_pred)


def test_more_groups_than_lanes_and_overlapping_groups():
    """G = 300 > 256: a lane takes a second group; classes in two groups; an empty group in the middle (a NaN mean, which
    wins the argmax as it does in torch)."""
    C, B = 600, 5
    groups = [[2 * g, (2 * g + 2) % C] for g in range(300)]          # class 2g + 2 closes group g and opens group g + 1
    rng = np.random.default_rng(4)
    z = rng.standard_normal((B, C)).astype(np.float32)
    y = rng.integers(0, C, B)
    check_both_modes(groups, C, torch.from_numpy(z), y, map_of(groups, C), map_of(groups, C))
    groups[40] = []
    got = accumulate(groups, C, torch.from_numpy(z), y, map_of(groups, C), map_of(groups, C), R.GROUP_MEAN)
    want = R.accumulate(z, y, map_of(groups, C), map_of(groups, C), groups, R.GROUP_MEAN)
    assert np.array_equal(got[2], want[2]) and (got[2] == 40).all() and np.array_equal(got[1], want[1])


def test_largest_label_set():
    """C = 21,841: groups of 10,000 / 11,000 / 500 members span several staging chunks each."""
    C, B = 21841, 3
    groups = scattered_groups(C, (10000, 11000, 500), 5)
    rng = np.random.default_rng(6)
    z = rng.standard_normal((B, C)).astype(np.float32)
    y = np.array([groups[0][0], groups[2][1], groups[1][5]])
    map_pred = map_of(groups, C)
    check_both_modes(groups, C, torch.from_numpy(z), y, map_pred, map_pred)
    gs = rng.standard_normal((B, 3)).astype(np.float32)
    gz = _C.group_logits_backward(_C.groups_handle(groups, C, 0), torch.from_numpy(gs).to(DEV)).cpu().numpy()
    assert same_bits(gz, R.group_logits_backward(gs, groups, C))


# ------------------------------------------------------------------------------------------------ targets, masks, ties
def test_unmapped_and_invalid_targets_count_nowhere(small):
    z16, _, _ = small
    z = torch.from_numpy(z16[:8, :10].copy())
    map_target = [-1] * 200
    for mode in MODES:
        totals, confusion, pred = accumulate(CIFAR_GROUPS, 10, z, np.arange(8), map_target, CIFAR_MAP, mode)
        assert totals.tolist() == [0, 0] and not confusion.any()
        assert np.array_equal(pred, R.predictions(z16[:8, :10], mode, CIFAR_MAP, CIFAR_GROUPS))      # written all the same
        map_one = [0] * 200
        y = np.array([-1, 200, 3, 2 ** 40, -2 ** 40, 7, 199, 0])
        totals, confusion, _ = accumulate(CIFAR_GROUPS, 10, z, y, map_one, CIFAR_MAP, mode)
        assert totals[0] == 4 and confusion.sum() == 4 and not confusion[1].any()


def test_masked_mode_below_minus_100():
    z = torch.full((4, 10), -200.0)
    z[:, [1, 9]] = 50.0                                 # unmapped classes: masked to -100, which still beats -200
    y = np.array([0, 1, 2, 3])
    totals, confusion, pred = accumulate(CIFAR_GROUPS, 10, z, y, [0, 1, 0, 1], CIFAR_MAP, R.MASKED)
    assert pred.tolist() == [-1] * 4 and totals.tolist() == [4, 0] and not confusion.any()
    z[2, 5] = -100.0                                    # a mapped logit AT -100 ties with the mask at class 1: the first wins
    z[3, 0] = -100.0                                    # ... and here the mapped class 0 comes first
    _, _, pred = accumulate(CIFAR_GROUPS, 10, z, y, [0, 1, 0, 1], CIFAR_MAP, R.MASKED)
    assert pred.tolist() == [-1, -1, -1, 1]


def test_ties_take_the_first_maximum():
    z = torch.zeros(3, 10)
    z[1, [4, 8]] = 5.0                                  # equal logits: class 4 (animal) before class 8 (vehicle)
    z[2, [8, 3]] = 5.0
    y = np.zeros(3, dtype=np.int64)
    _, _, pred = accumulate(CIFAR_GROUPS, 10, z, y, [0], CIFAR_MAP, R.MASKED)
    assert pred.tolist() == [1, 0, 0]                   # row 0: all equal, class 0 is a vehicle
    _, _, pred = accumulate(CIFAR_GROUPS, 10, z, y, [0], CIFAR_MAP, R.GROUP_MEAN)
    assert pred.tolist() == [0, 1, 1]                   # equal group means (0, 0) -> the first group; rows 1, 2: 5/6 < 5/2
    z = torch.zeros(1, 10)
    z[0, 2], z[0, 0] = 6.0, 2.0                         # means 6 / 6 and 2 / 2
    assert same_bits(_C.group_logits(_C.groups_handle(CIFAR_GROUPS, 10, 0), z.to(DEV)).cpu().numpy(), [[1.0, 1.0]])
    assert accumulate(CIFAR_GROUPS, 10, z, [0], [1], CIFAR_MAP, R.GROUP_MEAN)[2].tolist() == [0]


# ------------------------------------------------------------------------------------------------ the tree kernels
def test_group_logits_equal_the_root_columns_of_node_outputs():
    tree = Tree("CIFAR10", hierarchy="induced-ResNet18")
    flat = tree.flat
    b, e = int(flat.node_off[flat.root]), int(flat.node_off[flat.root + 1])
    groups = [flat.slot_cls[flat.slot_off[s]:flat.slot_off[s + 1]].tolist() for s in range(b, e)]
    assert sorted(c for g in groups for c in g) == list(range(10))
    z = torch.randn(257, 10, generator=torch.Generator().manual_seed(1)).to(DEV)
    node = _C.node_outputs(tree.device_handle(0), z)[0][:, b:e].cpu().numpy()
    got = _C.group_logits(_C.groups_handle(groups, 10, 0), z).cpu().numpy()
    assert same_bits(got, node) and same_bits(got, R.group_logits(z.cpu().numpy(), groups))


# ------------------------------------------------------------------------------------------------ accumulation
def test_two_calls_on_the_halves_equal_one_on_the_whole_and_runs_repeat(small):
    z16, y, map_target = small
    z = torch.from_numpy(z16[:, :10].copy())
    for mode in MODES:
        whole = accumulate(CIFAR_GROUPS, 10, z, y, map_target, CIFAR_MAP, mode)
        again = accumulate(CIFAR_GROUPS, 10, z, y, map_target, CIFAR_MAP, mode)
        totals = torch.zeros(2, dtype=torch.int64, device=DEV)
        confusion = torch.zeros(4, dtype=torch.int64, device=DEV)
        first = accumulate(CIFAR_GROUPS, 10, z[:131], y[:131], map_target, CIFAR_MAP, mode, totals, confusion)
        halves = accumulate(CIFAR_GROUPS, 10, z[131:], y[131:], map_target, CIFAR_MAP, mode, totals, confusion)
        for a, b, c in zip(whole, again, halves):
            assert np.array_equal(a, b)
        assert np.array_equal(whole[0], halves[0]) and np.array_equal(whole[1], halves[1])
        assert np.array_equal(whole[2], np.concatenate([first[2], halves[2]]))
        assert whole[0][0] == sum(0 <= v < 200 and map_target[v] >= 0 for v in y.tolist())


# ------------------------------------------------------------------------------------------------ backward
OVERLAP = [[0, 3, 5, 6], [3, 1], [7], [6, 3, 0, 9, 2, 1, 5, 8]]        # class 3 in three groups, 6 in two, 4 in none; sizes 4 2 1 8


def test_backward_matches_the_restatement_and_writes_every_element():
    handle = _C.groups_handle(OVERLAP, 10, 0)
    rng = np.random.default_rng(8)
    gs = rng.standard_normal((37, 4)).astype(np.float32)
    gs_d = torch.from_numpy(gs).to(DEV)
    gz = torch.full((37, 10), float("nan"), device=DEV)               # through the raw binding: nothing may stay NaN
    _C.check(_C.lib().nbdt_group_logits_backward(handle.h, _C.ptr(gs_d), 37, _C.ptr(gz), _C.stream_of(gs_d)))
    gz = gz.cpu().numpy()
    assert not np.isnan(gz).any() and same_bits(gz, R.group_logits_backward(gs, OVERLAP, 10))
    assert np.array_equal(bits(gz[:, 4]), np.zeros(37, dtype=np.uint32))              # a class in no group: exactly +0
    assert same_bits(gz, _C.group_logits_backward(handle, gs_d).cpu().numpy())


def test_forward_and_backward_equal_torch_on_exact_fixtures():
    g = torch.Generator().manual_seed(9)
    z = torch.randint(-1023, 1024, (19, 10), generator=g).float().to(DEV).requires_grad_(True)
    gs = torch.randint(-64, 65, (19, 4), generator=g).float().to(DEV)
    want = torch.stack([z[:, members].mean(dim=1) for members in OVERLAP], dim=1)
    want.backward(gs)
    want_gz, z.grad = z.grad.clone(), None
    got = EmbeddedDecisionRules.get_node_logits(z, new_to_old_classes=dict(enumerate(OVERLAP)), num_classes=4)
    got.backward(gs)
    assert same_bits(got.detach().cpu().numpy(), want.detach().cpu().numpy())
    assert same_bits(z.grad.cpu().numpy(), want_gz.cpu().numpy())
    assert same_bits(z.grad.cpu().numpy(), R.group_logits_backward(gs.cpu().numpy(), OVERLAP, 10))


# ------------------------------------------------------------------------------------------------ get_node_logits
def test_get_node_logits_with_an_ad_hoc_mapping():
    mapping = defaultdict(list)
    for old, new in enumerate(CIFAR_MAP):
        mapping[new].append(old)                                       # has a -1 key, like Superclass.build_mapping's
    mapping[7] = [1]                                                   # outside range(num_classes): ignored
    z = torch.randn(12, 10, generator=torch.Generator().manual_seed(2)).to(DEV).requires_grad_(True)
    out = EmbeddedDecisionRules.get_node_logits(z, new_to_old_classes=mapping, num_classes=2)
    assert out.shape == (12, 2) and out.requires_grad
    assert same_bits(out.detach().cpu().numpy(), R.group_logits(z.detach().cpu().numpy(), CIFAR_GROUPS))
    out.sum().backward()
    assert same_bits(z.grad.cpu().numpy(), R.group_logits_backward(np.ones((12, 2), np.float32), CIFAR_GROUPS, 10))
    assert set(mapping) == {-1, 0, 1, 7}                               # the defaultdict was not grown by the look-ups
    bf = EmbeddedDecisionRules.get_node_logits(z.detach().bfloat16(), new_to_old_classes=mapping, num_classes=2)
    assert bf.dtype == torch.float32 and same_bits(
        bf.cpu().numpy(), R.group_logits(R.bf16_round(z.detach().cpu().numpy()), CIFAR_GROUPS))
    holes = EmbeddedDecisionRules.get_node_logits(z.detach(), new_to_old_classes={0: [1], 2: [4, 5]}, num_classes=3)
    holes = holes.cpu().numpy()
    assert np.isnan(holes[:, 1]).all() and not np.isnan(holes[:, [0, 2]]).any()          # an empty group: a NaN column
    assert _C.groups_handle(CIFAR_GROUPS, 10, 0) is _C.groups_handle([tuple(g) for g in CIFAR_GROUPS], 10, 0)   # cached


def test_the_handle_cache_is_bounded():
    first = _C.groups_handle([[0], [1, 2]], 70, 0)
    assert _C.groups_handle([[0], [1, 2]], 70, 0) is first
    for c in range(_C.GROUPS_CACHE_MAX):                       # that many other groupings push the first one out
        _C.groups_handle([[c], [c + 1, c + 2]], 71, 0)
    assert len(_C._groups_cache) == _C.GROUPS_CACHE_MAX
    again = _C.groups_handle([[0], [1, 2]], 70, 0)
    assert again is not first and again.groups == first.groups
    z = torch.arange(70, dtype=torch.float32, device=DEV).reshape(1, 70)
    assert _C.group_logits(first, z).cpu().tolist() == [[0.0, 1.5]]      # an evicted handle lives as long as its holder
    assert _C.group_logits(again, z).cpu().tolist() == [[0.0, 1.5]]


# ------------------------------------------------------------------------------------------------ the analyzers
def hypernym_table():
    from nbdt.tree import get_wnids
    from nbdt.utils import dataset_to_default_path_wnids, hierarchy_to_path_graph
    table = {}
    for dataset in ("CIFAR10", "TinyImagenet200"):
        table.update(S.graph_hypernyms(get_wnids(dataset_to_default_path_wnids(dataset)),
                                       hierarchy_to_path_graph(dataset, "wordnet")))
    return table


@pytest.fixture(scope="module")
def analyzers():
    tree = Tree("CIFAR10", hierarchy="induced-ResNet18")
    kwargs = dict(tree=tree, superclass_wnids=["n00015388", "n04524313"], dataset_test="TinyImagenet200",
                  hypernyms=hypernym_table())
    return S.Superclass(**kwargs), S.SuperclassNBDT(**kwargs)


def test_analyzers_count_what_the_restatement_counts(analyzers, small, capsys):
    z16, y, _ = small
    z = torch.from_numpy(z16[:, :10].copy()).to(DEV)
    yd = torch.from_numpy(y).to(DEV)
    for a, mode in zip(analyzers, MODES):
        a.verbose = True
        want_t, want_c, want_p = R.accumulate(z16[:, :10], y, a.mapping_target.tolist(), a.mapping_pred.tolist(), a.groups, mode)
        with a.epoch_context(0):
            a.start_test(0)
            for lo in range(0, 300, 100):
                assert a.update_batch(z[lo:lo + 100], yd[lo:lo + 100], None) is None
            assert (a.total, a.correct) == tuple(want_t.tolist()) and np.array_equal(a.confusion(), want_c)
            assert a.accuracy() == 100.0 * want_t[1] / want_t[0]
            state = a.state()
            a.end_test(0)
        assert f"[{a.name}] Accuracy: {round(a.accuracy(), 2)}% ({want_t[1]} of {want_t[0]} " in capsys.readouterr().out
        pred, target = a.forward(z, yd)
        assert np.array_equal(pred.cpu().numpy(), want_p) and (a.total, a.correct) == tuple(want_t.tolist())
        assert target.cpu().tolist() == [a.mapping_target[v].item() if 0 <= v < 200 else -1 for v in y.tolist()]
        a.start_test(1)                                             # a new pass starts from zero ...
        assert (a.total, a.correct) == (0, 0) and not a.confusion().any()
        a.load_state(a.merge([state, state]))                       # ... and adopts a merged state on the device
        assert a.total == 2 * want_t[0] and np.array_equal(a.confusion(), 2 * want_c)
        a.sync_every_batch = True
        assert a.update_batch(z[:10], yd[:10]).startswith(a.name + ": ")
        a.sync_every_batch = False
        a.end_test(1)


def test_update_batch_does_not_synchronise_the_host(analyzers, small):
    z16, y, _ = small
    z = torch.from_numpy(z16[:100, :10].copy()).to(DEV)
    yd = torch.from_numpy(y[:100]).to(DEV)
    scalar = torch.ones((), device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            int(scalar)
            bites = False
        except RuntimeError:
            bites = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not bites:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag int(device_scalar) on this build")
    for a in analyzers:
        a.to(DEV)                                                   # the mappings and counters go up front, outside the pass
        a.start_test(0)
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(3):
                assert a.update_batch(z, yd, None) is None
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert a.total == 3 * R.accumulate(z16[:100, :10], y[:100], a.mapping_target.tolist(), a.mapping_pred.tolist(),
                                           a.groups, a.mode)[0][0]
        a.end_test(0)


def test_refusals_on_the_device():
    handle = _C.groups_handle(CIFAR_GROUPS, 10, 0)
    z = torch.zeros(4, 10, device=DEV)
    y = torch.zeros(4, dtype=torch.int64, device=DEV)
    totals = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(_C.NBDTHipError, match="columns"):
        _C.group_logits(handle, torch.zeros(4, 11, device=DEV))
    with pytest.raises(_C.NBDTHipError, match="map_target"):
        _C.superclass_accumulate(handle, z, y, torch.zeros(5, dtype=torch.int64, device=DEV), dev_i32(CIFAR_MAP), 0, totals)
    rc = _C.lib().nbdt_superclass_accumulate(handle.h, _C.ptr(z), 0, 4, 10, _C.ptr(y), _C.ptr(dev_i32([0])), 1, None,
                                             R.MASKED, _C.ptr(totals), None, None, _C.stream_of(z))
    assert rc == -1 and "map_pred" in _C.lib().nbdt_last_error().decode()
    rc = _C.lib().nbdt_superclass_accumulate(handle.h, _C.ptr(z), 0, 4, 10, _C.ptr(y), _C.ptr(dev_i32([0])), 1, None,
                                             7, _C.ptr(totals), None, None, _C.stream_of(z))
    assert rc == -1 and "mode" in _C.lib().nbdt_last_error().decode()
    torch.cuda.synchronize()
    assert totals.tolist() == [0, 0]
