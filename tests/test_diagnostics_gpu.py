"""nbdt_tree_stats_accumulate and nbdt.diagnostics on the MI355X against the numpy restatement of
tests/test_diagnostics.py (golden vectors of the reference) and against oracle/nbdt_oracle.py on larger batches.

Integer counters are compared exactly.  The soft rules' argmax is compared exactly on the rows whose top-2 gap in the
reference path probabilities is at least 1e-4 (the project's tolerance on P is rtol 2e-5 / atol 1e-6); the entropy sums
at the node-entropy tolerance of tests/test_rules_gpu.py (rtol 1e-4 / atol 1e-6, twice the rtol for the squares)."""
import ctypes

import numpy as np
import pytest
import torch

import nbdt_oracle as O
from conftest import GOLDEN_CASES
from test_diagnostics import ONE, load_case, restate, restate_golden, soft_gap_rows

pytestmark = pytest.mark.gpu

from nbdt import _C, diagnostics, ops  # noqa: E402
from nbdt.tree import Tree  # noqa: E402

DEV = "cuda:0"
EXACT = ("totals", "confusion_net", "confusion_hard", "node_counts", "first_error_depth")
# rows of each golden file whose soft top-2 gap is below 1e-4 (counted on the CPU from the golden soft_P)
SOFT_SKIPS = {"cifar100_wordnet": 2, "cifar100_wrn": 1, "cifar10_r18": 1, "cifar10_wordnet": 1, "cifar10_wrn": 1,
              "imagenet_eff": 0, "tiny_r18": 1, "tiny_wordnet": 0}


def _block(handle, fill=0, fields=ops.STATS_FIELDS):
    sizes = ops.tree_stats_sizes(handle)
    return {f: torch.full((sizes[f],), fill, dtype=torch.int64, device=DEV) for f in fields}


def _run(handle, z, y, fields=ops.STATS_FIELDS, scores=False, block=None):
    block = _block(handle, fields=fields) if block is None else block
    z, y = torch.as_tensor(z).to(DEV), torch.as_tensor(y).to(DEV)
    s = torch.full((z.shape[0], 3), -7.0, device=DEV) if scores else None
    ops.tree_stats_accumulate(handle, z, y, block, s)
    out = {k: v.cpu().numpy() for k, v in block.items()}
    return (out, s.cpu().numpy()) if scores else out


def _same(got, want, fields):
    for f in fields:
        assert np.array_equal(got[f], np.asarray(want[f]).ravel()), f


def _check_against(handle, want_of, z, y, node_entropy, soft_P, max_skipped):
    """One launch with everything requested against the restatement `want_of(rows)`."""
    got = _run(handle, z, y)
    want = want_of(np.arange(len(y)))
    t = want["totals"].copy()
    t[3] = got["totals"][3]                      # the soft hits are compared on the gapped rows below
    _same(got, {**want, "totals": t}, EXACT)
    safe = soft_gap_rows(soft_P)
    print("soft rows skipped:", int((~safe).sum()), "of", len(y))
    assert int((~safe).sum()) <= max_skipped
    rows = np.nonzero(safe)[0]
    got_safe = _run(handle, z[rows], y[rows], fields=("totals", "confusion_soft"))
    _same(got_safe, want_of(rows), ("totals", "confusion_soft"))
    # on the whole batch the soft counters may differ from the restatement by the skipped rows at most
    assert np.abs(got["confusion_soft"] - want["confusion_soft"].ravel()).sum() <= 2 * int((~safe).sum())
    valid = int(want["totals"][0])
    ent = np.asarray(node_entropy, dtype=np.float32)
    sums = got["node_entropy"].reshape(-1, 2) / float(ONE) / valid
    print("entropy mean max |err|", np.abs(sums[:, 0] - ent.mean(0, dtype=np.float64)).max())
    np.testing.assert_allclose(sums[:, 0], ent.mean(0, dtype=np.float64), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(sums[:, 1], (ent.astype(np.float64) ** 2).mean(0), rtol=2e-4, atol=1e-6)
    return got


@pytest.mark.parametrize("tag", list(GOLDEN_CASES))
def test_kernel_equals_the_restatement_on_the_golden_vectors(tag):
    g, tree, struct = load_case(tag)
    handle = tree.device_handle(0)
    assert handle.max_depth + 1 == len(restate_golden(g, struct)["first_error_depth"])

    def want_of(rows):
        return restate(struct, g["z"][rows], g["y"][rows], g["node_preds"][rows], g["node_entropy"][rows],
                       g["hard_pred"][rows], g["soft_P"][rows])
    _check_against(handle, want_of, g["z"], g["y"], g["node_entropy"], g["soft_P"], SOFT_SKIPS[tag])


# Gaussian logits, seeds chosen on the CPU so that the oracle's own soft_P leaves out at most 0.1 % of the rows.  At
# 1000 classes a node logit averages hundreds of leaves: with a standard deviation of 3 every node is close to uniform,
# the path products are tiny and about 0.6 % of the rows have an absolute top-2 gap below 1e-4 whatever the seed
# (seeds 1-11 counted); a standard deviation of 10 gives decided nodes.
LARGE = [("cifar100_wrn", 4096, 3.0, 7, 2), ("imagenet_eff", 2048, 10.0, 2, 0)]


@pytest.mark.parametrize("tag,B,std,seed,skipped", LARGE)
def test_larger_batch_equals_the_oracle(tag, B, std, seed, skipped, pkg_dir):
    g, tree, struct = load_case(tag)
    ds, h = GOLDEN_CASES[tag]
    otree = O.OracleTree(*O.default_paths(ds, h, pkg_dir))
    C = struct["C"]
    gen = torch.Generator().manual_seed(seed)
    z = (torch.randn(B, C, generator=gen) * std).numpy()
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(seed + 100)).numpy()
    y[::9] = z.argmax(1)[::9]                    # some backbone hits, so that every counter moves
    outs = O.node_outputs(otree, z)
    preds = np.stack([o["preds"] for o in outs], 1)
    ent = np.stack([o["entropy"] for o in outs], 1)
    hard, P = O.hard_forward(otree, z, outs), O.soft_forward(otree, z, outs)
    assert int((~soft_gap_rows(P)).sum()) == skipped and skipped <= B // 1000

    def want_of(rows):
        return restate(struct, z[rows], y[rows], preds[rows], ent[rows], hard[rows], P[rows])
    got = _check_against(tree.device_handle(0), want_of, z, y, ent, P, skipped)
    assert got["totals"][0] == B and got["totals"][1] >= B // 9


def _seeded(C, B, seed=5):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, generator=gen) * 3, torch.randint(0, C, (B,), generator=gen)


@pytest.mark.parametrize("ds,h", [("CIFAR100", "induced-wrn28_10_cifar100"), ("CIFAR10", "wordnet"),
                                  ("Imagenet1000", "induced-efficientnet_b7b")])
def test_accumulation_does_not_depend_on_the_batch_split(ds, h):
    tree = Tree(ds, hierarchy=h)
    handle = tree.device_handle(0)
    B = 1000 if len(tree.classes) <= 100 else 300
    z, y = _seeded(len(tree.classes), B)
    y[3], y[B // 2] = -1, len(tree.classes)
    once = _run(handle, z, y)
    assert once["totals"][0] == B - 2 and once["first_error_depth"].sum() == B - 2

    def split(order, sizes):
        block, at = _block(handle), 0
        for n in sizes:
            rows = order[at:at + n]
            _run(handle, z[rows], y[rows], block=block)
            at += n
        assert at == B
        return {k: v.cpu().numpy() for k, v in block.items()}
    _same(split(torch.arange(B), [B // 4] * 4), once, ops.STATS_FIELDS)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1))
    ragged = [B // 3, 17, B // 2, B - B // 3 - 17 - B // 2]
    _same(split(perm, ragged), once, ops.STATS_FIELDS)                    # the fixed-point entropy sums included
    twice = _block(handle)
    _run(handle, z, y, block=twice)
    both = _run(handle, z, y, block=twice)
    _same(both, {k: 2 * v for k, v in once.items()}, ops.STATS_FIELDS)


def test_null_pointers_invalid_labels_and_narrow_logits():
    g, tree, struct = load_case("cifar100_wrn")
    handle = tree.device_handle(0)
    full = _run(handle, g["z"], g["y"])
    # each statistic alone gives what it gives in company, and nothing else is touched
    for f in ops.STATS_FIELDS:
        block = _block(handle, fill=0)
        block = {k: (v if k == f else torch.full_like(v, 55)) for k, v in block.items()}
        ops.tree_stats_accumulate(handle, torch.from_numpy(g["z"]).to(DEV), torch.from_numpy(g["y"]).to(DEV), {f: block[f]})
        assert np.array_equal(block[f].cpu().numpy(), full[f]), f
        assert all((v == 55).all().item() for k, v in block.items() if k != f)
    # labels of -1 and C count nowhere
    y = g["y"].copy()
    y[0], y[5], y[-1] = -1, 100, 100
    keep = np.ones(len(y), bool)
    keep[[0, 5, len(y) - 1]] = False
    _same(_run(handle, g["z"], y), _run(handle, g["z"][keep], g["y"][keep]), ops.STATS_FIELDS)
    none = _run(handle, g["z"][:3], np.array([-1, 100, -5]))
    assert all((v == 0).all() for v in none.values())
    # bf16 / fp16 logits are up-cast on load: the same counters as their fp32 values
    for dt in (torch.bfloat16, torch.float16):
        zl = torch.from_numpy(g["z"]).to(dt)
        got, s = _run(handle, zl, g["y"], scores=True)
        want, sw = _run(handle, zl.float(), g["y"], scores=True)
        _same(got, want, ops.STATS_FIELDS)
        assert np.array_equal(s, sw)
    # a column slice of a wider matrix is consumed in place
    wide = torch.zeros(32, 128)
    wide[:, :100] = torch.from_numpy(g["z"])
    _same(_run(handle, wide.to(DEV)[:, :100], g["y"]), full, ops.STATS_FIELDS)
    # scores alone need no labels and no counters
    s = torch.empty(32, 3, device=DEV)
    ops.tree_stats_accumulate(handle, torch.from_numpy(g["z"]).to(DEV), None, None, s)
    assert np.array_equal(s.cpu().numpy(), _run(handle, g["z"], g["y"], scores=True)[1])
    # an empty batch is fine and counts nothing
    empty = _run(handle, torch.empty(0, 100), torch.empty(0, dtype=torch.long))
    assert all((v == 0).all() for v in empty.values())


def test_bad_arguments_fail_before_any_launch():
    g, tree, _ = load_case("cifar10_wrn")
    handle = tree.device_handle(0)
    z, y = torch.from_numpy(g["z"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    block = _block(handle, fill=123456789)
    scores = torch.full((64, 3), -7.0, device=DEV)
    st = _C.TreeStats()
    for name, t in block.items():
        setattr(st, name, t.data_ptr())
    lib, p = _C.lib(), _C.ptr
    call = lambda h, zz, zt, B, ld, yy: lib.nbdt_tree_stats_accumulate(  # noqa: E731
        h, zz, zt, B, ld, yy, ctypes.byref(st), p(scores), None)
    assert call(None, p(z), 0, 64, 10, p(y)) == -1 and b"null tree handle" in lib.nbdt_last_error()
    assert call(handle.h, None, 0, 64, 10, p(y)) == -1 and b"null logits" in lib.nbdt_last_error()
    assert call(handle.h, p(z), 7, 64, 10, p(y)) == -1 and b"dtype" in lib.nbdt_last_error()
    assert call(handle.h, p(z), 0, 64, 9, p(y)) == -1 and b"row stride" in lib.nbdt_last_error()
    assert call(handle.h, p(z), 0, -1, 10, p(y)) == -1
    assert call(handle.h, p(z), 0, 64, 10, None) == -1 and b"labels" in lib.nbdt_last_error()
    assert lib.nbdt_tree_stats_accumulate(handle.h, p(z), 0, 64, 10, p(y), None, None, None) == -1
    assert b"nothing requested" in lib.nbdt_last_error()
    torch.cuda.synchronize()
    assert all((v == 123456789).all().item() for v in block.values()) and (scores == -7.0).all().item()
    # the Python wrapper refuses what it can see
    with pytest.raises(_C.NBDTHipError, match="int64"):
        ops.tree_stats_accumulate(handle, z, y, {"totals": torch.zeros(4, device=DEV)})
    with pytest.raises(_C.NBDTHipError, match="unknown statistic"):
        ops.tree_stats_accumulate(handle, z, y, {"total": torch.zeros(4, dtype=torch.long, device=DEV)})
    with pytest.raises(_C.NBDTHipError, match="classes"):
        ops.tree_stats_accumulate(handle, z[:, :9], y, {})
    with pytest.raises(_C.NBDTHipError, match="scores"):
        ops.tree_stats_accumulate(handle, z, y, {}, torch.zeros(64, 2, device=DEV))


@pytest.mark.parametrize("tag", list(GOLDEN_CASES))
def test_scores_equal_torch_on_the_cpu(tag):
    g, tree, struct = load_case(tag)
    _, s = _run(tree.device_handle(0), g["z"], g["y"], fields=("totals",), scores=True)
    z = torch.from_numpy(g["z"])
    probs = torch.softmax(z, dim=1)
    h = torch.distributions.Categorical(probs=probs).entropy().numpy()
    top = torch.sort(probs, dim=1).values
    diff = (top[:, -1] - top[:, -2]).numpy()
    print("entropy max |err|", np.abs(s[:, 0] - h).max(), "top difference max |err|", np.abs(s[:, 1] - diff).max())
    np.testing.assert_allclose(s[:, 0], h, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(s[:, 1], diff, rtol=1e-4, atol=1e-6)
    # the reference's decision list opens with the root at entropy 0, then one entry per node of the walk
    for i in range(4):
        on = g["dec_path"][i] >= 0
        assert on.sum() < 32                                           # the recorded walk is complete
        ent = np.concatenate([[0.0], g["dec_entropy"][i][on]]).astype(np.float32)
        np.testing.assert_allclose(s[i, 2], ent.max() - ent.min(), rtol=1e-4, atol=1e-6)
    # and for every row: the spread of the golden node entropies over the walk through the golden node decisions
    for b in range(len(g["y"])):
        n, ents = struct["root"], [np.float32(0.0)]
        while n >= 0:
            ents.append(g["node_entropy"][b, n])
            n = struct["next"][n][int(g["node_preds"][b, n])]
        np.testing.assert_allclose(s[b, 2], max(ents) - min(ents), rtol=1e-4, atol=1e-6)


def test_tree_statistics_and_confusion_matrix_end_to_end(capsys, monkeypatch):
    g, tree, struct = load_case("cifar100_wrn")
    launches, real = [], ops.tree_stats_accumulate
    monkeypatch.setattr(ops, "tree_stats_accumulate", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    want = restate_golden(g, struct)
    ts = diagnostics.TreeStatistics(tree=tree)
    net, hard = diagnostics.ConfusionMatrix(tree.classes), diagnostics.ConfusionMatrix(tree=tree)
    soft = diagnostics.ConfusionMatrix(tree=tree, kind="soft")
    chain = diagnostics.Chain(ts, net, hard, soft)
    z, y = torch.from_numpy(g["z"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    with chain.epoch_context(1):
        chain.start_test(1)
        for rows in (slice(0, 12), slice(12, 24), slice(24, 32)):
            assert chain.update_batch(z[rows], y[rows], None) is None      # enqueues only: nothing to report yet
            assert ts._host is None and net._host is None                  # no transfer before an accessor asks
        chain.end_test(1)
    assert len(launches) == 3                    # four analyzers on one hierarchy, three batches: ONE launch per batch
    out = capsys.readouterr().out
    assert "[TreeStatistics] 32 samples" in out and "(diagonal)" in out
    got = ts.counts()
    _same(got, want, EXACT)
    assert np.array_equal(ts.confusion("net"), want["confusion_net"]) and np.array_equal(net.m, want["confusion_net"])
    assert np.array_equal(hard.m, want["confusion_hard"]) and np.array_equal(ts.confusion("hard"), hard.m)
    assert np.array_equal(soft.m, ts.confusion("soft"))
    assert np.abs(soft.m - want["confusion_soft"]).sum() <= 2 * SOFT_SKIPS["cifar100_wrn"]
    assert ts.first_error_histogram() == [int(v) for v in want["first_error_depth"]]
    rows = ts.node_table()
    assert [tuple(r[c] for c in diagnostics.COUNTERS) for r in rows] == [tuple(int(v) for v in c) for c in want["node_counts"]]
    np.testing.assert_allclose([r["entropy_mean"] for r in rows], g["node_entropy"].mean(0, dtype=np.float64),
                               rtol=1e-4, atol=1e-6)
    acc = ts.summary()["accuracy"]
    assert acc["net"] == 100.0 * want["totals"][1] / 32 and acc["hard"] == 100.0 * want["totals"][2] / 32
    assert np.allclose(np.nansum(net.recall(), 1)[want["confusion_net"].sum(1) > 0], 1.0)
    # a new pass starts from zero
    chain.start_epoch(2)
    chain.start_test(2)
    chain.update_batch(z[:5], y[:5], None)
    assert ts.totals()[0] == 5 and net.m.sum() == 5


def test_ranking_analyzers_keep_the_extreme_rows_of_a_pass():
    tree = Tree("CIFAR100", hierarchy="induced-wrn28_10_cifar100")
    z, y = _seeded(100, 257, seed=9)
    images = torch.arange(257, dtype=torch.float32).reshape(257, 1, 1, 1).expand(257, 3, 2, 2).contiguous()
    _, scores = _run(tree.device_handle(0), z, y, fields=("totals",), scores=True)
    analyzers = [diagnostics.Entropy(tree.classes, save_k=7), diagnostics.TopDifference(tree.classes, save_k=7),
                 diagnostics.NBDTEntropyMaxMin(tree=tree, save_k=7)]
    # the analyzers without a tree hand the kernel a one-level hierarchy: the backbone's scores do not depend on it
    chain = diagnostics.Chain(*analyzers)
    chain.verbose = False
    chain.start_epoch(0)
    chain.start_test(0)
    zd, yd, xd = z.to(DEV), y.to(DEV), images.to(DEV)
    for rows in (slice(0, 100), slice(100, 200), slice(200, 257)):
        assert chain.update_batch(zd[rows], yd[rows], xd[rows]) is None
    chain.end_test(0)
    with pytest.raises(ValueError, match="images"):           # images with every batch of a pass, or with none
        analyzers[1].update_batch(zd[:4], yd[:4])
    for a, col in zip(analyzers, (0, 1, 2)):
        order = np.argsort(scores[:, col], kind="stable")
        for kept, want in ((a.highest(), order[::-1][:7]), (a.lowest(), order[:7])):
            s, ordinal, img = (t.cpu().numpy() for t in kept)
            assert sorted(ordinal.tolist()) == sorted(want.tolist()), (a.name, ordinal, want)
            np.testing.assert_allclose(s, scores[ordinal, col], rtol=1e-5, atol=1e-7)
            assert np.array_equal(img[:, 0, 0, 0], ordinal.astype(np.float32))     # the image of that very sample
        assert (np.diff(a.highest()[0].cpu().numpy()) <= 0).all() and (np.diff(a.lowest()[0].cpu().numpy()) >= 0).all()
    h = scores[:, 0].astype(np.float64)
    for a in (analyzers[0], analyzers[2]):           # NBDTEntropyMaxMin keeps the backbone's statistics, as the reference
        assert abs(a.avg - h.mean()) < 1e-6 and abs(a.std - ((h - h.mean()) ** 2).sum()) < 1e-6 * max(a.std, 1.0)
    # without images nothing is kept for them
    lone = diagnostics.TopDifference(tree.classes, save_k=3)
    lone.start_epoch(0)
    lone.start_test(0)
    lone.update_batch(zd[:50], yd[:50])
    assert lone.highest()[2] is None and lone.highest()[0].shape == (3,)
