"""Rank-sharded device datasets and distributed evaluation on the MI355X.

A shard is defined by an explicit (rank, world), so one GPU plays every rank in turn: the batches of a shard are, bit for
bit, the batches the whole dataset returns for the same global indices (nbdt_augment_batch_sharded /
nbdt_resized_crop_batch_sharded: draw from the index, gather from index - lo); a shard holds its part of the bytes and no
more; the merged statistics of per-rank analyzers equal one analyzer fed the same batches; and a real two-rank run of
main.py --shard-data reports the whole split and keeps its replicas identical."""
import importlib.util
import json
import math
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import nbdt_path
from nbdt import analysis, data, diagnostics, models
from nbdt.tree import Tree

pytestmark = pytest.mark.gpu

spec = importlib.util.spec_from_file_location("nbdt_main", os.path.join(nbdt_path.PKG_DIR, "main.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

N = 37                       # odd: the shards are uneven at world 2 and 3
MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)
SEED, EPOCH = 11, 3
WORLDS = (1, 2, 3)


def _make(kind, shard=None):
    g = torch.Generator().manual_seed(5)
    y = torch.randint(0, 10, (N,), generator=g)
    if kind == "crop":
        x = torch.randint(0, 256, (N, 3, 20, 24), generator=g, dtype=torch.uint8)
        return data.ResizedCropDataset(x, y, MEAN, STD, size=16, resize=18, shard=shard)
    x = torch.randint(0, 256, (N, 3, 8, 8), generator=g, dtype=torch.uint8)
    if kind == "f32":
        x = torch.randn(N, 3, 8, 8, generator=g)
    return data.DeviceDataset(x, y, MEAN, STD, pad=2, shard=shard)


@pytest.fixture(scope="module")
def whole():
    """kind -> {train: (img, targets)} of the unsharded dataset for every index, computed once and only read."""
    out = {}
    everything = torch.arange(N)
    for kind in ("u8", "f32", "crop"):
        ds = _make(kind)
        assert ds.global_size == N and tuple(ds.shard_range) == (0, N) and ds.shape[0] == N
        out[kind] = {train: tuple(t.cpu() for t in ds.batch(everything, epoch=EPOCH, seed=SEED, train=train))
                     for train in (True, False)}
    return out


@pytest.mark.parametrize("train", (True, False), ids=("train", "eval"))
@pytest.mark.parametrize("kind", ("u8", "f32", "crop"))
def test_sharded_batches_are_the_unsharded_batches(whole, kind, train):
    want_img, want_y = whole[kind][train]
    for world in WORLDS:
        for rank in range(world):
            lo, hi = data.shard_range(N, rank, world)
            ds = _make(kind, shard=(rank, world))
            assert tuple(ds.shard_range) == (lo, hi) and ds.global_size == N
            assert ds.shape[0] == len(ds) == hi - lo and tuple(ds.shape[1:]) == ((3, 20, 24) if kind == "crop" else (3, 8, 8))
            owned = torch.arange(lo, hi)                    # rebased: 0 for the first, hi - 1 - lo for the last
            for index in (owned, owned.flip(0)[::2], owned.cuda()):      # host and device index tensors, any order
                img, y = ds.batch(index, epoch=EPOCH, seed=SEED, train=train)
                assert torch.equal(img.cpu(), want_img[index.cpu()]), (kind, train, world, rank)
                assert torch.equal(y.cpu(), want_y[index.cpu()]), (kind, train, world, rank)


@pytest.mark.parametrize("kind", ("u8", "crop"))
def test_the_draw_is_the_global_index_s(kind):
    """The parameters a shard reports are draw_params / draw_resized_crop_params of the GLOBAL index."""
    lo, hi = data.shard_range(N, 2, 3)
    ds = _make(kind, shard=(2, 3))
    index = torch.arange(lo, hi)
    used = ds.batch(index, epoch=EPOCH, seed=SEED, return_params=True)[2].cpu().numpy()
    if kind == "crop":
        want = data.draw_resized_crop_params(SEED, EPOCH, index, 20, 24)
    else:
        want = data.draw_params(SEED, EPOCH, index, 2)
    assert np.array_equal(used, np.stack(want, axis=1))
    rebased = data.draw_params(SEED, EPOCH, index - lo, 2) if kind == "u8" else \
        data.draw_resized_crop_params(SEED, EPOCH, index - lo, 20, 24)
    assert not np.array_equal(used, np.stack(rebased, axis=1))          # (the test could tell the difference)


@pytest.mark.parametrize("kind", ("u8", "f32", "crop"))
def test_an_index_outside_the_shard_is_refused_or_blanked(kind):
    lo, hi = data.shard_range(N, 1, 3)
    ds = _make(kind, shard=(1, 3))
    for bad in (lo - 1, hi, 0, N - 1, -1, N):
        with pytest.raises(ValueError, match=rf"\[{lo}, {hi}\)"):
            ds.batch(torch.tensor([lo, bad]))
    # a device index tensor cannot be checked on the host: the kernel writes a zero image with label -1 and reads nothing
    index = torch.tensor([lo, lo - 1, hi, hi - 1, -1, N, 0, -2 ** 63, 2 ** 63 - 1]).cuda()
    for train in (True, False):
        img, y = ds.batch(index, epoch=EPOCH, seed=SEED, train=train)
        ok = torch.tensor([True, False, False, True, False, False, False, False, False])
        assert (y.cpu()[~ok] == -1).all() and (y.cpu()[ok] >= 0).all()
        assert (img.cpu()[~ok] == 0).all() and img.cpu()[ok].abs().sum() > 0


def test_a_shard_holds_its_part_of_the_bytes():
    x = torch.zeros(64, 3, 32, 32, dtype=torch.uint8)
    y = torch.zeros(64, dtype=torch.long)
    for rank in range(4):
        ds = data.DeviceDataset(x, y, MEAN, STD, pad=4, shard=(rank, 4))
        assert tuple(ds.shape) == (16, 3, 32, 32) and ds.x.is_cuda and tuple(ds.shard_range) == (16 * rank, 16 * rank + 16)
        assert ds.x.untyped_storage().nbytes() == 16 * 3 * 32 * 32
        assert ds.y.untyped_storage().nbytes() == 16 * 8
    rc = data.ResizedCropDataset(x, y, MEAN, STD, size=16, resize=18, shard=(3, 4))
    assert tuple(rc.shape) == (16, 3, 32, 32) and rc.x.untyped_storage().nbytes() == 16 * 3 * 32 * 32


# ------------------------------------------------------------------------------------------------------------
# evaluation over shards equals evaluation over the split

SPLIT = 250


@pytest.fixture(scope="module")
def setup():
    device = torch.device("cuda", 0)
    net = models.ResNet10(num_classes=10, device=device, seed=0)
    tree = Tree("CIFAR10", hierarchy="induced-ResNet10")
    g = torch.Generator().manual_seed(21)
    y = torch.randint(0, 10, (SPLIT,), generator=g)
    x = torch.randint(0, 256, (SPLIT, 3, 32, 32), generator=g, dtype=torch.uint8)
    return device, net, tree, x, y


def _analyzer(tree):
    return diagnostics.Chain(analysis.HardEmbeddedDecisionRules(tree=tree), diagnostics.TreeStatistics(tree=tree),
                             diagnostics.ConfusionMatrix(tree.classes), diagnostics.Entropy(tree.classes))


def _dataset(x, y, device, shard=None):
    stats = data.DATASET_STATS["CIFAR10"]
    return data.DeviceDataset(x, y, stats["mean"], stats["std"], stats["pad"], device=device, shard=shard)


@pytest.mark.parametrize("world", (2, 3))
def test_merged_rank_evaluations_equal_one_evaluation(setup, world):
    device, net, tree, x, y = setup
    crit = nn.CrossEntropyLoss()
    # every rank on its own shard with its own analyzer ...
    states, hits, seen, loss, batches = [], 0, 0, 0.0, 0
    for rank in range(world):
        a = _analyzer(tree)
        a.start_test(0)
        plain, loss_sum, nb = M.evaluate_part(net, crit, a, 1, _dataset(x, y, device, (rank, world)), None, 100, device,
                                              rank, world)
        states.append(a.state())
        hits, seen, loss, batches = hits + int(plain.hits), seen + plain.seen, loss + float(loss_sum), batches + nb
    merged = _analyzer(tree)
    merged.start_test(0)
    merged.load_state(merged.merge(states))
    # ... against ONE analyzer fed the same per-rank batches in the same order (no kernel sees another shape), and an
    # Entropy that keeps every sample's score, for the terms of the floating sums
    one, every = _analyzer(tree), diagnostics.Entropy(tree.classes, save_k=SPLIT)
    one.start_test(0)
    every.start_test(0)
    whole = _dataset(x, y, device)
    ref_hits, ref_seen, ref_loss, ref_batches = 0, 0, 0.0, 0
    for rank in range(world):
        plain, loss_sum, nb = M.evaluate_part(net, crit, one, 1, whole, None, 100, device, rank, world)
        M.evaluate_part(net, crit, every, 1, whole, None, 100, device, rank, world)
        ref_hits, ref_seen, ref_loss, ref_batches = (ref_hits + int(plain.hits), ref_seen + plain.seen,
                                                     ref_loss + float(loss_sum), ref_batches + nb)
    assert seen == ref_seen == SPLIT and hits == ref_hits and batches == ref_batches
    assert batches == sum(math.ceil((hi - lo) / 100) for lo, hi in (data.shard_range(SPLIT, r, world) for r in range(world)))
    # the loss sum: fp32 batch means, one per batch, added in fp32 -- terms x eps x sum of magnitudes (all positive)
    assert abs(loss - ref_loss) <= batches * torch.finfo(torch.float32).eps * abs(ref_loss)
    rules, stats, cm, ent = merged.analyzers
    rules1, stats1, cm1, ent1 = one.analyzers
    # integers: exactly
    assert (rules.correct, rules.total) == (rules1.correct, rules1.total) and rules.total == SPLIT
    assert rules.accuracy() == rules1.accuracy()
    for field in stats1.fields:
        assert np.array_equal(stats.counts()[field], stats1.counts()[field]), field
    assert stats.totals()[0] == SPLIT and stats.totals()[1] == hits and stats.totals()[2] == rules.correct
    assert np.array_equal(cm.m, cm1.m) and cm.m.sum() == SPLIT
    assert np.array_equal(cm.m, stats.confusion("net"))
    # the rankings: the same samples, by their index in the whole split, in the same order, with the same scores
    for got, want in ((ent.highest(), ent1.highest()), (ent.lowest(), ent1.lowest())):
        assert got[1].tolist() == want[1].tolist() and len(got[1]) == ent.save_k
        assert torch.equal(got[0].cpu(), want[0].cpu())
    assert ent.report()["samples"] == SPLIT
    # floating accumulators: within the reordering bound of their own dtype, computed from the terms themselves
    assert ent._sums.dtype == ent1._sums.dtype == diagnostics.SUMS_DTYPE
    h = every.highest()[0].to(diagnostics.SUMS_DTYPE).cpu()
    assert h.numel() == SPLIT
    eps = torch.finfo(diagnostics.SUMS_DTYPE).eps
    for j, terms in enumerate((h, h * h)):
        bound = SPLIT * eps * float(terms.abs().sum())
        diff = abs(float(ent._sums[j]) - float(ent1._sums[j]))
        print(f"world {world} sums[{j}]: merged {float(ent._sums[j])!r} one {float(ent1._sums[j])!r} diff {diff:.3e} "
              f"bound {bound:.3e}")
        assert diff <= bound


# ------------------------------------------------------------------------------------------------------------
# a two-rank run of main.py

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _two_ranks(tmp_path, tag, argv):
    """main.py argv on two ranks: fresh child processes, each under its own time limit; when one fails the other is not
    left waiting for it.  Returns rank 0's stdout."""
    from concurrent.futures import ThreadPoolExecutor, as_completed
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_shard_rank_worker.py")
    port = _free_port()
    logs = [(open(tmp_path / f"{tag}{r}.out", "w"), open(tmp_path / f"{tag}{r}.err", "w")) for r in range(2)]
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", str(port), str(tmp_path / f"{tag}{r}")] + argv,
                              cwd=tmp_path, stdout=logs[r][0], stderr=logs[r][1]) for r in range(2)]

    def wait(p):
        try:
            return p.wait(timeout=240)
        except subprocess.TimeoutExpired:
            return "timeout"
    try:
        with ThreadPoolExecutor(2) as pool:
            for done in as_completed([pool.submit(wait, p) for p in procs]):
                if done.result() != 0:
                    for p in procs:
                        if p.poll() is None:
                            p.kill()
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for files in logs:
            for f in files:
                f.close()
    for r, p in enumerate(procs):
        assert p.returncode == 0, (r, p.returncode, (tmp_path / f"{tag}{r}.err").read_text()[-3000:])
    return (tmp_path / f"{tag}0.out").read_text()


EVAL = ("--eval --synthetic 256 --arch ResNet10 --dataset CIFAR10 --augment reference --shard-data "
        "--analysis HardEmbeddedDecisionRules --diagnostics TreeStatistics").split()


def test_two_rank_evaluation_reports_the_whole_split(tmp_path):
    out = _two_ranks(tmp_path, "eval", EVAL + ["--diagnostics-out", "diag.json"])
    report = json.loads((tmp_path / "diag.json").read_text())["TreeStatistics"]
    # the same split, model and batches in this process: each rank's shard through evaluate_part
    args = M.parse_args(EVAL)
    device = torch.device("cuda", 0)
    _, _, test_x, test_y = M.load_data(args, 10, device, raw=True)
    net = models.ResNet10(num_classes=10, device=device, seed=args.seed)
    tree = Tree("CIFAR10", hierarchy="induced-ResNet10")
    totals, correct, plain_hits = np.zeros(4, dtype=np.int64), 0, 0
    for rank in range(2):
        a = diagnostics.Chain(analysis.HardEmbeddedDecisionRules(tree=tree), diagnostics.TreeStatistics(tree=tree))
        a.start_test(0)
        plain, _, _ = M.evaluate_part(net, nn.CrossEntropyLoss(), a, 1, _dataset(test_x, test_y, device, (rank, 2)), None,
                                      100, device, rank, 2)
        totals += np.asarray(a.analyzers[1].totals())
        correct += a.analyzers[0].correct
        plain_hits += int(plain.hits)
        assert a.analyzers[1].totals()[0] == test_x.shape[0] // 2         # a rank saw its half
    n = test_x.shape[0]
    assert report["totals"][0] == n == 512                                 # all test samples, not half
    assert report["totals"] == totals.tolist() and totals[1] == plain_hits and totals[2] == correct
    hits = re.search(r"\[NBDT-Hard\] rules accuracy ([0-9.]+)% \((\d+) of (\d+)\)", out)
    assert hits and (int(hits.group(2)), int(hits.group(3))) == (correct, n)
    acc = re.search(r"\| Acc: ([0-9.]+)%", out)
    assert acc and acc.group(1) == "%.3f" % (100.0 * plain_hits / n)
    results = [json.loads((tmp_path / f"eval{r}.json").read_text()) for r in range(2)]
    assert results[0] == results[1] and results[0]["acc"] == 100.0 * plain_hits / n      # every rank holds the reduction
    assert "--shard-data: rank 0 of 2 holds train samples (0, 128) and test samples (0, 256)" in out


def test_two_rank_sharded_training_keeps_replicas_identical(tmp_path):
    out = _two_ranks(tmp_path, "train", ("--synthetic 256 --arch ResNet10 --dataset CIFAR10 --augment reference "
                                         "--shard-data --batch-size 128 --epochs 1 --lr 0.05").split())
    loss = re.search(r"Loss: ([0-9.naninf-]+) \((\d+) steps of 2 x 64 images\)", out)
    assert loss and int(loss.group(2)) == 2 and math.isfinite(float(loss.group(1))), out[-2000:]
    flat = [torch.load(tmp_path / f"train{r}.pt") for r in range(2)]
    assert torch.isfinite(flat[0]).all() and torch.equal(flat[0], flat[1])
    results = [json.loads((tmp_path / f"train{r}.json").read_text()) for r in range(2)]
    assert results[0] == results[1] and 0.0 <= results[0]["acc"] <= 100.0
