"""nbdt.diagnostics without a GPU: the public surface, the report arithmetic on a hand-written block of counters, and a
numpy restatement of everything nbdt_tree_stats_accumulate counts, built from the reference's golden vectors and checked
for self-consistency on all eight hierarchies.  tests/test_diagnostics_gpu.py compares the kernel with `restate`."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import nbdt_path
from conftest import GOLDEN_CASES
from nbdt import _C, analysis, diagnostics, ops
from nbdt.tree import Tree

ONE = 1 << 32          # fixed-point unit of the entropy sums
COUNTERS = ("on_path", "on_path_right", "visited", "visited_on_path", "visited_on_path_right")


# ------------------------------------------------------------------------------------------------------------
# numpy restatement

def golden_structure(g):
    """The reference Tree's maps as recorded in a rules_*.npz: per inner node (sorted wnid order) the leaf-class set of
    every child and where the child leads (inner node index, or -(class) - 1)."""
    wnids = [str(w) for w in g["tree_inode_wnids"]]
    index = {w: i for i, w in enumerate(wnids)}
    leaves = {str(w): i for i, w in enumerate(g["tree_wnids_leaves"])}
    child_off, slot_off, slot_cls = g["tree_child_off"], g["tree_slot_off"], g["tree_slot_cls"]
    sets, nxt = [], []
    for n in range(len(wnids)):
        sets.append([set(int(c) for c in slot_cls[slot_off[s]:slot_off[s + 1]]) for s in range(child_off[n], child_off[n + 1])])
        nxt.append([index[str(w)] if str(w) in index else -leaves[str(w)] - 1
                    for w in g["tree_child_wnid"][child_off[n]:child_off[n + 1]]])
    return {"wnids": wnids, "root": index[str(g["tree_root"])], "sets": sets, "next": nxt, "C": len(leaves)}


def longest_walk(struct):
    """Inner nodes on the longest root-to-leaf walk (nbdt_tree_max_depth)."""
    memo = {}

    def depth(n):
        if n not in memo:
            memo[n] = 1 + max([depth(c) for c in struct["next"][n] if c >= 0], default=0)
        return memo[n]
    return depth(struct["root"])


def restate(struct, z, y, node_preds, node_entropy, hard_pred, soft_P):
    """Everything the kernel counts, by the definitions of include/nbdt_hip.h, sample by sample."""
    C, N, D = struct["C"], len(struct["wnids"]), longest_walk(struct)
    out = {"totals": np.zeros(4, np.int64), "node_counts": np.zeros((N, 5), np.int64),
           "node_entropy": np.zeros((N, 2), np.int64), "first_error_depth": np.zeros(D + 1, np.int64),
           "confusion_net": np.zeros((C, C), np.int64), "confusion_hard": np.zeros((C, C), np.int64),
           "confusion_soft": np.zeros((C, C), np.int64)}
    net, soft = np.argmax(z, axis=1), np.argmax(soft_P, axis=1)          # numpy: the first maximum
    ent = np.asarray(node_entropy, dtype=np.float32)
    fixed = np.rint(ent.astype(np.float64) * ONE).astype(np.int64)
    fixed_sq = np.rint((ent * ent).astype(np.float64) * ONE).astype(np.int64)      # the square is rounded to fp32 first
    for b in range(len(y)):
        label = int(y[b])
        if not 0 <= label < C:
            continue                                                       # counts nowhere
        out["totals"] += (1, net[b] == label, hard_pred[b] == label, soft[b] == label)
        out["confusion_net"][label, net[b]] += 1
        out["confusion_hard"][label, hard_pred[b]] += 1
        out["confusion_soft"][label, soft[b]] += 1
        out["node_entropy"][:, 0] += fixed[b]
        out["node_entropy"][:, 1] += fixed_sq[b]
        right = np.zeros(N, bool)
        under = np.zeros(N, bool)
        for n in range(N):
            under[n] = any(label in s for s in struct["sets"][n])
            right[n] = label in struct["sets"][n][int(node_preds[b, n])]
        out["node_counts"][:, 0] += under
        out["node_counts"][:, 1] += right
        n, d, first = struct["root"], 0, None
        while True:
            out["node_counts"][n, 2:] += (1, under[n], right[n])
            if first is None and not right[n]:
                first = d
            n = struct["next"][n][int(node_preds[b, n])]
            d += 1
            if n < 0:
                break
        assert -n - 1 == hard_pred[b], "the walk over node_preds ends at the golden hard prediction"
        out["first_error_depth"][D if first is None else first] += 1
    return out


def soft_gap_rows(soft_P, gap=1e-4):
    """Rows whose soft argmax is safe to compare exactly: top-1 minus top-2 path probability of at least `gap` (the
    project's tolerance on P is rtol 2e-5 / atol 1e-6, so a smaller gap may legitimately flip)."""
    top = np.sort(np.asarray(soft_P, dtype=np.float64), axis=1)
    return (top[:, -1] - top[:, -2]) >= gap


def load_case(tag):
    ds, h = GOLDEN_CASES[tag]
    g = np.load(os.path.join(nbdt_path.ROOT, "tests", "golden", f"rules_{tag}.npz"))
    return g, Tree(ds, hierarchy=h), golden_structure(g)


def restate_golden(g, struct):
    return restate(struct, g["z"], g["y"], g["node_preds"], g["node_entropy"], g["hard_pred"], g["soft_P"])


@pytest.mark.parametrize("tag", list(GOLDEN_CASES))
def test_restatement_is_self_consistent(tag):
    g, tree, struct = load_case(tag)
    flat = tree.flat
    # the golden maps are this repository's Tree (inner nodes sorted by wnid, children in link order)
    assert struct["wnids"] == flat.inode_wnids and struct["root"] == flat.root
    assert [len(s) for s in struct["sets"]] == list(np.diff(flat.node_off))
    assert [c for per in struct["next"] for c in per] == list(flat.slot_next)
    r = restate_golden(g, struct)
    t = r["totals"]
    assert t[0] == len(g["y"])
    for i, kind in enumerate(("net", "hard", "soft")):
        assert np.trace(r["confusion_" + kind]) == t[1 + i] and r["confusion_" + kind].sum() == t[0]
    assert r["first_error_depth"].sum() == t[0]
    assert r["first_error_depth"][-1] == t[2]                # never leaving the path = a hard-rules hit
    counts = r["node_counts"]
    assert counts[struct["root"], 2] == t[0] and counts[struct["root"], 0] == t[0]
    assert (counts[:, 1] <= counts[:, 0]).all() and (counts[:, 4] <= counts[:, 3]).all()
    assert (counts[:, 3] <= counts[:, 2]).all() and (counts[:, 3] <= counts[:, 0]).all()
    for n in range(len(struct["wnids"])):
        inner = sum(counts[c, 3] for c in struct["next"][n] if c >= 0)
        leaf_hits = sum(r["confusion_hard"][-c - 1, -c - 1] for c in struct["next"][n] if c < 0)
        assert counts[n, 4] == inner + leaf_hits, (tag, n)


# ------------------------------------------------------------------------------------------------------------
# public surface

def test_header_declares_the_entry_point_and_the_version_moved():
    text = open(os.path.join(nbdt_path.ROOT, "include", "nbdt_hip.h")).read()
    assert "int nbdt_tree_stats_accumulate(" in text and "typedef struct nbdt_tree_stats {" in text
    for field in _C.TreeStats.FIELDS:
        assert f"int64_t* {field};" in text
    assert "nbdt_tree_stats_accumulate" in _C.SIGNATURES
    assert _C.lib().nbdt_version() >= 112
    # argument checks come before any device work: callable without a GPU
    assert _C.lib().nbdt_tree_stats_accumulate(None, None, 0, 4, 10, None, None, None, None) == -1
    assert b"null tree handle" in _C.lib().nbdt_last_error()


def test_names():
    assert diagnostics.names == ("TreeStatistics", "ConfusionMatrix", "Entropy", "TopDifference", "NBDTEntropyMaxMin")
    assert analysis.names == ("Noop", "HardEmbeddedDecisionRules", "SoftEmbeddedDecisionRules")
    for name in diagnostics.names:
        assert issubclass(getattr(diagnostics, name), analysis.Noop)
    assert issubclass(diagnostics.Chain, analysis.Noop)


class _Recorder(analysis.Noop):
    def __init__(self, log, tag, fail_in=None):
        super().__init__(("a", "b"))
        self.log, self.tag, self.fail_in = log, tag, fail_in
        for hook in ("start_epoch", "end_epoch", "start_train", "end_train", "start_test", "end_test"):
            setattr(self, hook, self._hook(hook))

    def _hook(self, hook):
        def call(epoch):
            self.log.append((self.tag, hook, epoch))
            if hook == self.fail_in:
                raise RuntimeError(hook)
        return call

    def update_batch(self, outputs, targets, images=None):
        self.log.append((self.tag, "update_batch", images))
        return self.tag


def test_chain_calls_every_hook_of_every_member_in_order():
    log = []
    chain = diagnostics.Chain(_Recorder(log, 0), _Recorder(log, 1), _Recorder(log, 2))
    assert chain.classes == ("a", "b") and chain.name == "Noop"
    with chain.epoch_context(3):
        chain.start_train(3)
        chain.end_train(3)
        chain.start_test(3)
        assert chain.update_batch("z", "y", "x") == 0          # the first member's statistic
        chain.end_test(3)
    hooks = ["start_epoch", "start_train", "end_train", "start_test", "update_batch", "end_test", "end_epoch"]
    assert [(t, h) for t, h, _ in log] == [(t, h) for h in hooks for t in (0, 1, 2)]
    assert all(e == ("x" if h == "update_batch" else 3) for _, h, e in log)
    chain.verbose = False
    assert [a.verbose for a in chain.analyzers] == [False] * 3


def test_chain_runs_end_hooks_when_a_body_or_a_member_raises():
    log = []
    chain = diagnostics.Chain(_Recorder(log, 0), _Recorder(log, 1))

    @chain.test_function
    def body(epoch):
        raise KeyError("body")

    chain.start_epoch(0)
    with pytest.raises(KeyError):
        body(0)
    assert [(t, h) for t, h, _ in log][-2:] == [(0, "end_test"), (1, "end_test")]
    log.clear()
    chain = diagnostics.Chain(_Recorder(log, 0, fail_in="end_test"), _Recorder(log, 1))
    with pytest.raises(RuntimeError, match="end_test"):
        chain.end_test(0)
    assert [(t, h) for t, h, _ in log] == [(0, "end_test"), (1, "end_test")]     # the second member still ran


def test_main_parser_knows_the_diagnostics_flags():
    spec = importlib.util.spec_from_file_location("nbdt_main_diag", os.path.join(nbdt_path.PKG_DIR, "main.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    p = M.build_parser()
    a = p.parse_args(["--analysis", "HardEmbeddedDecisionRules", "--diagnostics", "TreeStatistics", "ConfusionMatrix",
                      "--diagnostics-out", "f.json"])
    assert a.diagnostics == ["TreeStatistics", "ConfusionMatrix"] and a.diagnostics_out == "f.json"
    assert a.analysis == "HardEmbeddedDecisionRules"
    assert p.parse_args([]).diagnostics == [] and p.parse_args([]).diagnostics_out is None
    with pytest.raises(SystemExit):
        p.parse_args(["--diagnostics", "TopEntropy"])
    with pytest.raises(SystemExit):
        p.parse_args(["--analysis", "TreeStatistics"])          # --analysis keeps its own choices
    # a training run cannot carry ConfusionMatrix (its start_train raises, as the reference's): refused up front
    assert M.parse_args(["--eval", "--diagnostics", "ConfusionMatrix"]).diagnostics == ["ConfusionMatrix"]
    assert M.parse_args(["--diagnostics", "TreeStatistics", "Entropy"]).eval is False
    with pytest.raises(SystemExit):
        M.parse_args(["--diagnostics", "TreeStatistics", "ConfusionMatrix"])
    with pytest.raises(SystemExit):
        M.parse_args(["--eval", "--diagnostics-out", "f.json"])


# ------------------------------------------------------------------------------------------------------------
# report arithmetic

def _hand_block(N, D):
    counts = np.zeros((N, 5), np.int64)
    counts[0] = (40, 30, 40, 40, 30)        # 75 % both ways
    counts[1] = (20, 5, 12, 8, 2)           # 25 % given arrival, 25 % over all
    counts[2] = (10, 9, 3, 0, 0)            # never reached on path: no support
    counts[3] = (7, 7, 9, 6, 3)             # 50 % given arrival
    ent = np.zeros((N, 2), np.int64)
    ent[0] = (int(0.5 * 40 * ONE), int(0.3 * 40 * ONE))        # mean 0.5, mean square 0.3 -> std sqrt(0.05)
    ent[1] = (int(0.25 * 40 * ONE), int(0.0625 * 40 * ONE))    # constant 0.25 -> std 0
    fed = np.zeros(D + 1, np.int64)
    fed[0], fed[1], fed[D] = 10, 8, 22
    return {"totals": np.array([40, 30, 22, 24]), "node_counts": counts, "node_entropy": ent, "first_error_depth": fed}


def test_report_arithmetic_on_a_hand_written_block(tmp_path):
    ts = diagnostics.TreeStatistics(dataset="CIFAR10", hierarchy="induced-ResNet18", confusions=False)
    N = len(ts.tree.inodes)
    D = 1 + max(diagnostics.inode_depths(ts.tree))
    block = _hand_block(N, D)
    ts.load_counts(block)
    rows = ts.node_table()
    assert len(rows) == N and [r["wnid"] for r in rows] == [n.wnid for n in ts.tree.inodes]
    assert rows[ts.tree.flat.root]["depth"] == 0 and all(r["children"] == 2 for r in rows)
    assert {r["depth"] for r in rows} == set(range(D))
    for r, expect in zip(rows, block["node_counts"]):
        assert tuple(r[c] for c in COUNTERS) == tuple(expect)
    assert rows[0]["accuracy_given_arrival"] == 0.75 and rows[0]["accuracy_all"] == 0.75
    assert rows[1]["accuracy_given_arrival"] == 0.25 and rows[1]["accuracy_all"] == 0.25
    assert rows[3]["accuracy_given_arrival"] == 0.5 and rows[3]["accuracy_all"] == 1.0
    # zero support: nan, not a division error
    assert math.isnan(rows[2]["accuracy_given_arrival"]) and rows[2]["accuracy_all"] == 0.9
    assert math.isnan(rows[4]["accuracy_given_arrival"]) and math.isnan(rows[4]["accuracy_all"])
    assert abs(rows[0]["entropy_mean"] - 0.5) < 1e-9 and abs(rows[0]["entropy_std"] - math.sqrt(0.05)) < 1e-9
    assert abs(rows[1]["entropy_mean"] - 0.25) < 1e-9 and rows[1]["entropy_std"] < 1e-4
    assert rows[4]["entropy_mean"] == 0.0
    assert ts.first_error_histogram() == [10, 8] + [0] * (D - 2) + [22]
    s = ts.summary(k=2)
    assert s["samples"] == 40 and s["accuracy"] == {"net": 75.0, "hard": 55.0, "soft": 60.0}
    assert [r["index"] for r in s["worst_nodes"]] == [1, 3]
    assert [r["index"] for r in ts.summary(k=5, min_support=7)["worst_nodes"]] == [1, 0]       # node 3 has 6 arrivals
    with pytest.raises(RuntimeError, match="confusions"):
        ts.confusion("hard")
    with pytest.raises(ValueError):
        ts.confusion("other")
    # an empty pass: every ratio is nan
    ts.load_counts({k: np.zeros_like(v) for k, v in block.items()})
    assert all(math.isnan(v) for v in ts.summary()["accuracy"].values()) and ts.summary()["worst_nodes"] == []
    assert math.isnan(ts.node_table()[0]["entropy_mean"])

    # JSON round trip: strict JSON (nan -> null), the counters come back exactly
    ts.load_counts(block)
    path = tmp_path / "stats.json"
    ts.to_json(path)
    back = json.loads(path.read_text())
    assert back["totals"] == [40, 30, 22, 24] and back["accuracy"]["hard"] == 55.0
    assert back["first_error_depth"] == ts.first_error_histogram()
    assert back["nodes"][2]["accuracy_given_arrival"] is None and back["nodes"][0]["accuracy_given_arrival"] == 0.75
    again = diagnostics.TreeStatistics(tree=ts.tree, confusions=False).load_counts(
        {"totals": back["totals"], "first_error_depth": back["first_error_depth"], **back["counts"]})
    assert again.summary(k=2) == ts.summary(k=2)


def test_confusion_matrix_normalisation_and_contract():
    cm = diagnostics.ConfusionMatrix(("a", "b", "c"))
    assert cm.kind == "net" and cm.k == 3
    cm.load_counts({"confusion_net": [[3, 1, 0], [0, 0, 0], [2, 0, 2]]})
    assert np.array_equal(cm.m, [[3, 1, 0], [0, 0, 0], [2, 0, 2]])
    recall, precision = cm.recall(), cm.precision()
    assert np.allclose(recall[0], [0.75, 0.25, 0]) and np.isnan(recall[1]).all() and np.allclose(recall[2], [0.5, 0, 0.5])
    assert np.allclose(precision[:, 0], [0.6, 0, 0.4]) and np.allclose(precision[:, 2], [0, 0, 1])
    cm.start_epoch(0)
    with pytest.raises(NotImplementedError):
        cm.start_train(0)
    with pytest.raises(ValueError):
        diagnostics.ConfusionMatrix(("a", "b"), kind="hard")          # the rules' matrices need a tree
    tree = Tree("CIFAR10", hierarchy="induced-ResNet18")
    assert diagnostics.ConfusionMatrix(tree=tree).kind == "hard" and diagnostics.ConfusionMatrix(tree=tree).k == 10
    with pytest.raises(RuntimeError, match="no batch"):
        diagnostics.ConfusionMatrix(tree=tree).m


def test_cpu_logits_are_refused():
    z, y = torch.randn(4, 10), torch.zeros(4, dtype=torch.long)
    tree = Tree("CIFAR10", hierarchy="induced-ResNet18")
    for a in (diagnostics.TreeStatistics(tree=tree), diagnostics.ConfusionMatrix(tree.classes),
              diagnostics.Entropy(tree.classes), diagnostics.TopDifference(tree.classes),
              diagnostics.NBDTEntropyMaxMin(tree=tree)):
        a.start_epoch(0)
        a.start_test(0)
        with pytest.raises(_C.NBDTHipError):
            a.update_batch(z, y, None)
    with pytest.raises(_C.NBDTHipError):
        ops.tree_stats_accumulate(None, z, y, {})
