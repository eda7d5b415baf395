"""Host side of rank-sharded datasets and distributed evaluation (no GPU): the one rule that says which rank owns which
samples (nbdt.data.shard_range), the per-rank sampler (nbdt.dist.epoch_indices) and the pure merges behind the analyzers'
reduce()."""
import numpy as np
import pytest
import torch

from nbdt import analysis, data, diagnostics
from nbdt import dist as ndist

SIZES = (1, 7, 100, 50000)
WORLDS = (1, 2, 3, 8)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("world", WORLDS)
def test_shard_ranges_tile_the_dataset_evenly(n, world):
    ranges = [data.shard_range(n, r, world) for r in range(world)]
    assert ranges[0][0] == 0 and ranges[-1][1] == n
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))            # contiguous, in rank order
    sizes = [hi - lo for lo, hi in ranges]
    assert min(sizes) >= 0 and max(sizes) - min(sizes) <= 1 and sum(sizes) == n
    assert min(sizes) == n // world                                         # what the sharded sampler's step count uses
    if n < world:
        assert sizes.count(0) == world - n                                  # some ranks own nothing


def test_shard_range_refuses_a_rank_outside_the_world():
    for rank, world in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError, match="rank"):
            data.shard_range(10, rank, world)


@pytest.mark.parametrize("cls", ("DeviceDataset", "ResizedCropDataset"))
def test_datasets_refuse_an_empty_shard(cls):
    """n < world: the rank that owns nothing is told so before anything is moved to a device."""
    x, y = torch.zeros(2, 3, 8, 8, dtype=torch.uint8), torch.zeros(2, dtype=torch.long)
    empty = [r for r in range(3) if data.shard_range(2, r, 3)[0] == data.shard_range(2, r, 3)[1]]
    assert len(empty) == 1
    with pytest.raises(ValueError, match=r"owns none of the 2 samples.*empty shard"):
        if cls == "DeviceDataset":
            data.DeviceDataset(x, y, (0.5,) * 3, (0.2,) * 3, 2, shard=(empty[0], 3))
        else:
            data.ResizedCropDataset(x, y, (0.5,) * 3, (0.2,) * 3, size=4, resize=6, shard=(empty[0], 3))


@pytest.mark.parametrize("world", (1, 2, 4))
def test_unsharded_sampler_is_the_permutation_the_driver_always_cut(world):
    n, batch, seed, epoch = 1000, 64, 3, 5
    for rank in range(world):
        got = ndist.epoch_indices(n, batch, rank, world, seed, epoch, sharded=False)
        # the three lines of main.py's training loop before the sampler existed
        g = torch.Generator().manual_seed(seed * 1000 + epoch)
        perm = torch.randperm(n, generator=g)
        want = [ndist.shard_batch(perm[i * batch:(i + 1) * batch], rank, world) for i in range(n // batch)]
        assert got.dtype == torch.int64 and tuple(got.shape) == (n // batch, batch // world)
        assert torch.equal(got, torch.stack(want))


@pytest.mark.parametrize("n,batch,world", [(37, 6, 3), (100, 16, 2), (50000, 512, 8), (7, 2, 1), (9, 8, 8)])
def test_sharded_sampler_stays_inside_the_shard(n, batch, world):
    plans = [ndist.epoch_indices(n, batch, r, world, seed=1, epoch=4, sharded=True) for r in range(world)]
    steps = (n // world) // (batch // world)            # set by the smallest shard
    for r, plan in enumerate(plans):
        lo, hi = data.shard_range(n, r, world)
        assert plan.dtype == torch.int64 and tuple(plan.shape) == (steps, batch // world)      # equal on all ranks
        assert int(plan.min()) >= lo and int(plan.max()) < hi
        assert plan.unique().numel() == plan.numel()                                            # no repeat in the epoch


def test_sharded_sampler_depends_on_seed_epoch_and_rank_and_nothing_else():
    args = dict(n=4000, batch_size=64, world=2, seed=2, epoch=3, sharded=True)
    a = ndist.epoch_indices(rank=0, **args)
    assert torch.equal(a, ndist.epoch_indices(rank=0, **args))
    assert not torch.equal(a, ndist.epoch_indices(rank=0, **{**args, "epoch": 4}))
    assert not torch.equal(a, ndist.epoch_indices(rank=0, **{**args, "seed": 3}))
    # another rank does not walk its shard in the same order (both shards have 2000 samples here)
    b = ndist.epoch_indices(rank=1, **args)
    assert not torch.equal(a - data.shard_range(4000, 0, 2)[0], b - data.shard_range(4000, 1, 2)[0])


def test_sampler_refuses_a_batch_the_ranks_cannot_split():
    with pytest.raises(ValueError, match="divisible"):
        ndist.epoch_indices(100, 10, 0, 3, 0, 0, sharded=True)


# ------------------------------------------------------------------------------------------------------------
# merges

def test_merge_of_integer_states_is_a_sum():
    a = {"hits": 3, "seen": 10, "counts": {"totals": np.array([4, 1, 2, 3]), "confusion_net": np.arange(4).reshape(2, 2)}}
    b = {"hits": 5, "seen": 7, "counts": {"totals": np.array([1, 1, 1, 1]), "confusion_net": np.ones((2, 2), dtype=np.int64)}}
    c = {"hits": 0, "seen": 0, "counts": {}}                  # a rank that saw no batch has no counters
    got = analysis.merge_sum([a, b, c])
    assert got["hits"] == 8 and got["seen"] == 17
    assert got["counts"]["totals"].tolist() == [5, 2, 3, 4]
    assert got["counts"]["confusion_net"].tolist() == [[1, 2], [3, 4]]
    assert a["counts"]["totals"].tolist() == [4, 1, 2, 3]     # pure: the inputs are as they were
    # what the analyzers' own merge is made of (configuration only, no device)
    rules = analysis.HardEmbeddedDecisionRules(dataset="CIFAR10", hierarchy="induced")
    assert rules.merge([{"hits": 3, "seen": 10}, {"hits": 5, "seen": 7}]) == {"hits": 8, "seen": 17}
    cm = diagnostics.ConfusionMatrix(("a", "b"))
    merged = cm.merge([{"counts": {"confusion_net": np.array([1, 0, 2, 3])}},
                       {"counts": {"confusion_net": np.array([0, 5, 0, 1])}}])
    assert cm.load_counts(merged["counts"]).m.tolist() == [[1, 5], [2, 4]]


def test_reduce_is_a_no_op_without_a_process_group():
    rules = analysis.HardEmbeddedDecisionRules(dataset="CIFAR10", hierarchy="induced")
    rules.load_state({"hits": 4, "seen": 9})
    assert rules.reduce() is rules and (rules.correct, rules.total) == (4, 9)
    chain = diagnostics.Chain(rules, diagnostics.Entropy(rules.classes))
    assert chain.reduce() is chain


def _candidates(score, index):
    return {"score": torch.tensor(score, dtype=torch.float32), "index": torch.tensor(index), "images": None}


def _ranked(score, index, k, largest):
    """A rank's own top k of its samples under the ranking's order (what an analyzer retains)."""
    return diagnostics.merge_topk([_candidates(score, index)], k, largest)


@pytest.mark.parametrize("largest", (True, False))
def test_ranking_merge_breaks_ties_by_global_index_whatever_the_split(largest):
    # 12 samples; the extreme score is shared by samples 2, 5, 9 and 11, the next one by 0 and 7
    top, second = (4.0, 3.0) if largest else (-4.0, -3.0)
    score = [second, 0.5, top, 0.1, 0.2, top, 0.3, second, 0.4, top, 0.0, top]
    index = list(range(12))
    k = 5
    want = [2, 5, 9, 11, 0]              # ties: the smaller sample index first
    results = []
    for cuts in ([0, 12], [0, 6, 12], [0, 3, 10, 12]):             # 1, 2 and 3 states
        states = [_ranked(score[a:b], index[a:b], k, largest) for a, b in zip(cuts, cuts[1:])]
        got = diagnostics.merge_topk(states, k, largest)
        assert got["index"].tolist() == want, (cuts, got)
        assert got["score"].tolist() == [score[i] for i in want]
        results.append(got["index"].tolist())
    assert results[0] == results[1] == results[2]
    # the states' order does not matter either, and a rank without samples is skipped
    a, b = _ranked(score[:6], index[:6], k, largest), _ranked(score[6:], index[6:], k, largest)
    assert diagnostics.merge_topk([b, None, a], k, largest)["index"].tolist() == want


def test_ranking_analyzers_merge_their_states():
    ent = diagnostics.Entropy(("a", "b", "c"), save_k=2)
    s = [{"counts": {}, "seen": 3, "sums": torch.tensor([1.5, 2.0], dtype=diagnostics.SUMS_DTYPE),
          "highest": _candidates([2.0, 1.0], [1, 0]), "lowest": _candidates([0.5, 1.0], [2, 0])},
         {"counts": {}, "seen": 2, "sums": torch.tensor([0.25, 1.0], dtype=diagnostics.SUMS_DTYPE),
          "highest": _candidates([2.0, 0.5], [3, 4]), "lowest": _candidates([0.5, 2.0], [4, 3])}]
    m = ent.merge(s)
    assert m["seen"] == 5 and m["sums"].tolist() == [1.75, 3.0] and m["sums"].dtype == diagnostics.SUMS_DTYPE
    assert m["highest"]["index"].tolist() == [1, 3] and m["lowest"]["index"].tolist() == [2, 4]
    ent.load_state(m)
    assert ent.report()["samples"] == 5 and ent.avg == 1.75 / 5
    assert ent.highest()[1].tolist() == [1, 3] and ent.lowest()[0].tolist() == [0.5, 0.5]
    # images travel with their samples
    img = lambda ids: torch.tensor(ids, dtype=torch.float32).view(-1, 1, 1, 1).expand(-1, 3, 2, 2)   # noqa: E731
    a = {**_candidates([1.0, 0.0], [0, 1]), "images": img([0, 1])}
    b = {**_candidates([3.0, 1.0], [2, 3]), "images": img([2, 3])}
    got = diagnostics.merge_topk([a, b], 3, True)
    assert got["index"].tolist() == [2, 0, 3] and got["images"][:, 0, 0, 0].tolist() == [2.0, 0.0, 3.0]
    with pytest.raises(ValueError, match="images"):
        diagnostics.merge_topk([a, _candidates([1.0], [9])], 3, True)


def test_chain_merges_member_by_member_and_the_shared_block_once():
    classes = ("a", "b")
    make = lambda: diagnostics.Chain(diagnostics.ConfusionMatrix(classes), diagnostics.Entropy(classes, save_k=1))  # noqa
    chain = make()
    states = [{"shared": {"confusion_net": np.array([1, 0, 0, 2])},
               "members": [{"counts": None}, {"counts": None, "seen": 3, "sums": torch.tensor([1.0, 1.0]).double(),
                                              "highest": _candidates([0.5], [2]), "lowest": _candidates([0.1], [0])}]},
              {"shared": {"confusion_net": np.array([0, 4, 1, 0])},
               "members": [{"counts": None}, {"counts": None, "seen": 5, "sums": torch.tensor([2.0, 3.0]).double(),
                                              "highest": _candidates([0.5], [7]), "lowest": _candidates([0.2], [3])}]}]
    merged = chain.merge(states)
    assert merged["shared"]["confusion_net"].tolist() == [1, 4, 1, 2]
    chain.load_state(merged)
    cm, ent = chain.analyzers
    assert cm.m.tolist() == [[1, 4], [1, 2]]
    assert ent.report()["samples"] == 8 and ent.highest()[1].tolist() == [2] and ent.lowest()[1].tolist() == [0]


# ------------------------------------------------------------------------------------------------------------
# the C entries

@pytest.mark.parametrize("base,n", [(-1, 16), (-2 ** 63, 16), (2 ** 63 - 1, 16), (2 ** 63 - 16, 16), (1, 2 ** 63 - 1)])
def test_sharded_entries_refuse_an_index_base_that_could_wrap(base, n):
    """index_base < 0 or index_base + N past int64: refused before any HIP call (the pointers are never dereferenced).
    With such a base the kernel's unsigned comparison could take a far-away index for a row of the shard."""
    import ctypes
    from nbdt import _C
    lib = _C.lib()
    assert lib.nbdt_version() >= 114
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    f3, d2 = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_double * 2)(0.5, 1.0)
    rc = lib.nbdt_augment_batch_sharded(p, _C.NBDT_U8, p, p, base, 4, n, 32, 32, 4, 1, f3, f3, f3, 0, 0, None, p, p, None, None)
    assert rc == -1 and "index_base" in lib.nbdt_last_error().decode()
    rc = lib.nbdt_resized_crop_batch_sharded(p, _C.NBDT_U8, p, p, base, 4, n, 32, 32, 16, 16, 0, 0, 16, 16, 1, f3, f3, d2, d2,
                                             p, 0, 0, None, p, p, None, None)
    assert rc == -1 and "index_base" in lib.nbdt_last_error().decode()
