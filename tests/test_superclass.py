"""Host side of the superclass evaluation (no GPU): the class -> superclass mapping from its three sources, the label
subsets against the restatement of the reference's draw (tests/_superclass_ref.py), merge / load_state of the analyzers,
the driver's refusals, the sampler's subset and the C-ABI table."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import nbdt_path
from nbdt import _C
from nbdt import analysis
from nbdt import dist as ndist
from nbdt import superclass as S
from nbdt.data import label_subset, shard_range
from nbdt.model import EmbeddedDecisionRules
from nbdt.tree import Tree, get_wnids
from nbdt.utils import dataset_to_default_path_wnids

import _superclass_ref as R
import main as driver

ANIMAL, VEHICLE = "n00015388", "n04524313"
EINVAL = -1


def wnids_of(dataset):
    return get_wnids(dataset_to_default_path_wnids(dataset))


def graph_mapping(dataset, supers=(ANIMAL, VEHICLE)):
    with pytest.warns(UserWarning, match="LOSSY"):
        return S.Superclass.build_mapping(wnids_of(dataset), list(supers))


# ------------------------------------------------------------------------------------------------ the mapping
TABLE = {"a": ["a", "mammal", "animal"], "b": ["b", "car", "vehicle"], "c": ["c", "rock"], "d": ["d", "amphibious", "vehicle",
                                                                                                 "animal"], "animal": []}


def test_build_mapping_from_an_explicit_table(tmp_path):
    wnids = ["a", "b", "c", "d", "animal"]
    mapping, new_to_old = S.Superclass.build_mapping(wnids, ["animal", "vehicle"], TABLE)
    assert mapping.dtype == torch.int64 and mapping.tolist() == [0, 1, -1, 0, 0]      # the class itself is a hypernym
    assert dict(new_to_old) == {0: [0, 3, 4], 1: [1], -1: [2]}
    assert (mapping.tolist(), dict(new_to_old)) == R.build_mapping(wnids, ["animal", "vehicle"], TABLE)
    assert new_to_old[5] == []                                            # a defaultdict, as in the reference
    path = tmp_path / "hypernyms.json"
    path.write_text(json.dumps(TABLE))
    from_file, _ = S.Superclass.build_mapping(wnids, ["animal", "vehicle"], str(path))
    assert from_file.tolist() == mapping.tolist()
    with pytest.raises(KeyError, match="no entry"):
        S.Superclass.build_mapping(wnids + ["e"], ["animal"], TABLE)


def test_first_listed_superclass_wins_for_a_class_under_two():
    wnids = ["a", "b", "c", "d", "animal"]
    # d lies under both: it goes to whichever is listed first, whatever the order of its own hypernym list
    assert S.Superclass.build_mapping(wnids, ["animal", "vehicle"], TABLE)[0].tolist() == [0, 1, -1, 0, 0]
    assert S.Superclass.build_mapping(wnids, ["vehicle", "animal"], TABLE)[0].tolist() == [1, 0, -1, 0, 1]


@pytest.fixture
def no_wordnet(monkeypatch):
    """build_mapping as it runs where nltk's WordNet is not installed: the second source answers None."""
    monkeypatch.setattr(S, "wordnet_hypernyms", lambda wnids: None)


def test_graph_fallback_cifar10_vector_counts_and_warning(no_wordnet):
    mapping, new_to_old = graph_mapping("CIFAR10")
    assert mapping.tolist() == [1, -1, 0, 0, 0, 0, 0, 0, 1, -1]          # automobile and truck are lost (second parent)
    assert new_to_old[0] == [2, 3, 4, 5, 6, 7] and new_to_old[1] == [0, 8] and new_to_old[-1] == [1, 9]
    for dataset, animals, vehicles in (("CIFAR100", 43, 1), ("TinyImagenet200", 59, 2)):
        m = graph_mapping(dataset)[0].tolist()
        assert (m.count(0), m.count(1), len(m)) == (animals, vehicles, len(wnids_of(dataset)))


def test_graph_fallback_is_refused_without_a_shipped_graph(no_wordnet):
    with pytest.raises(RuntimeError, match="no hypernym source"):
        S.Superclass.build_mapping(["n00000001", "n00000002"], [ANIMAL])
    with pytest.raises(RuntimeError, match="no hypernym source"):          # Imagenet1000 ships no graph-wordnet.json
        S.Superclass.build_mapping(wnids_of("Imagenet1000"), [ANIMAL])


# ------------------------------------------------------------------------------------------------ label subsets
def fixture_labels(n=300, k=10, seed=5):
    return torch.randint(0, k, (n,), generator=torch.Generator().manual_seed(seed))


def test_label_subset_matches_the_restated_draw():
    y = fixture_labels()
    labels = y.tolist()
    ones = lambda keep: [int(c in keep) for c in range(10)]  # noqa: E731
    got = label_subset(y, 10, include_labels=[2, 7])
    assert got.dtype == torch.int64 and got.tolist() == R.label_subset(labels, ones({2, 7}))
    assert got.tolist() == [i for i, c in enumerate(labels) if c in (2, 7)]
    got = label_subset(y, 10, exclude_labels=[0, 1])
    assert got.tolist() == R.label_subset(labels, ones(set(range(2, 10)))) == [i for i, c in enumerate(labels) if c > 1]
    for seed in (0, 1):
        got = label_subset(y, 10, probability_labels=0.25, seed=seed).tolist()
        assert got == R.label_subset(labels, [0.25] * 10, seed) and got == sorted(got) and 30 < len(got) < 120
        assert got == label_subset(y, 10, probability_labels=[0.25], seed=seed).tolist()
    assert label_subset(y, 10, probability_labels=0.25, seed=0).tolist() != label_subset(y, 10, probability_labels=0.25,
                                                                                         seed=1).tolist()
    p = [0.0, 1.0, 0.5, 0.25, 0.75, 1.0, 0.0, 0.1, 0.9, 0.5]
    assert label_subset(y, 10, probability_labels=p, seed=3).tolist() == R.label_subset(labels, p, 3)
    names = [f"w{c}" for c in range(10)]
    assert label_subset(y, 10, include_classes=["w7", "w2"], classes=names).tolist() == \
        label_subset(y, 10, include_labels=[2, 7]).tolist()
    state = __import__("random").getstate()
    label_subset(y, 10, probability_labels=0.5)
    assert __import__("random").getstate() == state            # the process's generator is left alone


def test_label_subset_errors():
    y = fixture_labels()
    with pytest.raises(ValueError, match="Length of probabilities vector 3"):
        label_subset(y, 10, probability_labels=[0.5, 0.5, 0.5])
    with pytest.raises(ValueError, match="empty"):
        label_subset(y, 10, probability_labels=0.0)
    with pytest.raises(ValueError, match="empty"):
        label_subset(y, 10, include_labels=[])
    with pytest.raises(ValueError, match="exactly one"):
        label_subset(y, 10, include_labels=[1], exclude_labels=[2])
    with pytest.raises(ValueError, match="exactly one"):
        label_subset(y, 10)
    # a label outside [0, k) is named, not wrapped to the end of p or left to an IndexError
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 10\), got min -1"):
        label_subset(torch.tensor([3, -1, 4]), 10, probability_labels=1.0)
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 10\), got min 3, max 10"):
        label_subset(torch.tensor([3, 10, 4]), 10, include_labels=[3])


def test_epoch_indices_over_a_subset():
    y = fixture_labels(n=1000)
    kept = label_subset(y, 10, exclude_labels=[0, 1])
    allowed = set(kept.tolist())
    plan = ndist.epoch_indices(1000, 64, 0, 1, seed=0, epoch=3, subset=kept)
    flat = plan.reshape(-1).tolist()
    assert plan.shape == (kept.numel() // 64, 64) and set(flat) <= allowed and len(set(flat)) == len(flat)
    assert not torch.equal(plan, ndist.epoch_indices(1000, 64, 0, 1, seed=0, epoch=4, subset=kept))
    halves = [ndist.epoch_indices(1000, 64, r, 2, seed=0, epoch=3, subset=kept) for r in range(2)]
    assert torch.equal(torch.cat(halves, dim=1), plan)                    # the ranks cut the same global batches
    shards = [ndist.epoch_indices(1000, 64, r, 4, seed=0, epoch=3, sharded=True, subset=kept) for r in range(4)]
    assert len({tuple(s.shape) for s in shards}) == 1 and shards[0].shape[1] == 16
    for r, s in enumerate(shards):
        lo, hi = shard_range(1000, r, 4)
        flat = s.reshape(-1).tolist()
        assert set(flat) <= allowed and all(lo <= i < hi for i in flat) and len(set(flat)) == len(flat)
    with pytest.raises(ValueError, match="subset indices"):
        ndist.epoch_indices(10, 2, 0, 1, 0, 0, subset=torch.tensor([3, 10]))
    # no subset: the plan is what it always was
    g = torch.Generator().manual_seed(0 * 1000 + 3)
    assert torch.equal(ndist.epoch_indices(1000, 100, 0, 1, 0, 3), torch.randperm(1000, generator=g).view(10, 100))


# ------------------------------------------------------------------------------------------------ the analyzers, host side
def cifar_hypernyms():
    """An explicit table over CIFAR10 and TinyImagenet200 from the shipped graphs (what --superclass-file would hold)."""
    table = {}
    for dataset in ("CIFAR10", "TinyImagenet200"):
        from nbdt.utils import hierarchy_to_path_graph
        table.update(S.graph_hypernyms(wnids_of(dataset), hierarchy_to_path_graph(dataset, "wordnet")))
    return table


@pytest.fixture(scope="module")
def tree():
    return Tree("CIFAR10", hierarchy="induced-ResNet18")


def test_constructors_names_and_the_empty_superclass_refusal(tree):
    assert S.names == ("Superclass", "SuperclassNBDT")
    assert analysis.names == ("Noop", "HardEmbeddedDecisionRules", "SoftEmbeddedDecisionRules")
    table = cifar_hypernyms()
    a = S.Superclass(tree=tree, superclass_wnids=[ANIMAL, VEHICLE], dataset_test="TinyImagenet200", hypernyms=table,
                     metric="top5")
    assert isinstance(a, analysis.DecisionRules) and a.name == "Superclass" and a.accepts_superclass_wnids
    assert a.mapping_pred.tolist() == [1, -1, 0, 0, 0, 0, 0, 0, 1, -1] and a.groups == [[2, 3, 4, 5, 6, 7], [0, 8]]
    assert len(a.mapping_target) == 200 and len(a.mapped_classes) == 61 and a.dataset_test == "TinyImagenet200"
    assert (a.total, a.correct, a.accuracy()) == (0, 0, 0.0) and a.confusion().shape == (2, 2) and not a.sync_every_batch
    same = S.SuperclassNBDT(tree=tree, superclass_wnids=[ANIMAL, VEHICLE], hypernyms=table)
    assert same.name == "Superclass-NBDT" and same.dataset_test == "CIFAR10" and same.mapping_target.tolist() == \
        same.mapping_pred.tolist()
    S.Superclass(tree=tree, superclass_wnids=[ANIMAL, "n99999999"], hypernyms=table)       # the masked mode needs no member
    with pytest.raises(ValueError, match="n99999999"):
        S.SuperclassNBDT(tree=tree, superclass_wnids=[ANIMAL, "n99999999"], hypernyms=table)
    with pytest.raises(ValueError, match="at least one"):
        S.Superclass(tree=tree, superclass_wnids=[], hypernyms=table)


def test_merge_of_a_three_way_split_equals_the_whole(tree):
    table = cifar_hypernyms()
    a = S.SuperclassNBDT(tree=tree, superclass_wnids=[ANIMAL, VEHICLE], dataset_test="TinyImagenet200", hypernyms=table)
    rng = np.random.default_rng(7)
    z = rng.standard_normal((90, 10)).astype(np.float32)
    y = rng.integers(0, 200, 90)
    mt, mp = a.mapping_target.tolist(), a.mapping_pred.tolist()
    whole_t, whole_c, _ = R.accumulate(z, y, mt, mp, a.groups, R.GROUP_MEAN)
    assert 0 < whole_t[1] < whole_t[0] < 90
    states = []
    for lo, hi in ((0, 17), (17, 64), (64, 90)):
        t, c, _ = R.accumulate(z[lo:hi], y[lo:hi], mt, mp, a.groups, R.GROUP_MEAN)
        states.append({"totals": t, "confusion": c})
    merged = a.merge(states + [None])
    assert np.array_equal(merged["totals"], whole_t) and np.array_equal(merged["confusion"], whole_c)
    assert np.array_equal(states[0]["totals"], R.accumulate(z[:17], y[:17], mt, mp, a.groups, R.GROUP_MEAN)[0])   # pure
    a.load_state(merged)
    assert (a.total, a.correct) == (int(whole_t[0]), int(whole_t[1])) and np.array_equal(a.confusion(), whole_c)
    assert a.accuracy() == 100.0 * whole_t[1] / whole_t[0]
    assert np.array_equal(a.state()["totals"], whole_t) and np.array_equal(a.state()["confusion"], whole_c)
    empty = a.merge([])
    assert empty["totals"].tolist() == [0, 0] and empty["confusion"].shape == (2, 2)
    assert a.reduce() is a                                      # no process group: a no-op


def test_end_test_prints_the_reference_line(tree, capsys):
    a = S.Superclass(tree=tree, superclass_wnids=[ANIMAL, VEHICLE], hypernyms=cifar_hypernyms())
    a.start_test(0)
    a.load_state({"totals": np.array([8, 6]), "confusion": np.array([[5, 1], [1, 1]])})
    a.end_test(0)
    assert "[Superclass] Accuracy: 75.0% (6 of 8 " in capsys.readouterr().out
    a.verbose = False
    a.start_test(1)
    a.end_test(1)
    assert capsys.readouterr().out == "" and a.phase is None


def test_ad_hoc_get_node_logits_is_on_the_hip_path_now():
    with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):           # it used to be NotImplementedError
        EmbeddedDecisionRules.get_node_logits(torch.zeros(2, 10), new_to_old_classes={0: [1, 2], 1: [3]}, num_classes=2)


# ------------------------------------------------------------------------------------------------ the driver
BASE = ["--dataset", "CIFAR10", "--synthetic", "64", "--eval"]


def refused(argv, capsys, text):
    with pytest.raises(SystemExit):
        driver.parse_args(argv)
    assert text in capsys.readouterr().err


def test_parse_args_refusals_and_defaults(capsys):
    args = driver.parse_args(BASE)
    assert (args.dataset_test, args.data_file_test, args.disable_test_eval, args.superclass_wnids, args.superclass_file,
            args.include_labels, args.exclude_labels, args.probability_labels, args.include_classes, args.label_subset) == \
        (None, None, False, [], None, None, None, None, None, None)
    refused(BASE + ["--dataset-test", "TinyImagenet200"], capsys, "--disable-test-eval")
    refused(BASE + ["--data-file-test", "x.pth"], capsys, "needs --dataset-test")
    refused(BASE + ["--analysis", "Superclass"], capsys, "needs --superclass-wnids")
    refused(BASE + ["--superclass-wnids", ANIMAL], capsys, "belong to --analysis Superclass")
    refused(BASE + ["--include-labels", "1", "--exclude-labels", "2"], capsys, "pass one of them")
    refused(BASE + ["--exclude-labels"], capsys, "needs at least one value")
    train = ["--dataset", "CIFAR10", "--synthetic", "64"]
    refused(train + ["--disable-test-eval"], capsys, "needs an --analysis that reports an accuracy")
    refused(train + ["--disable-test-eval", "--analysis", "Noop"], capsys, "needs an --analysis that reports an accuracy")
    assert driver.parse_args(train + ["--disable-test-eval", "--analysis", "SoftEmbeddedDecisionRules"]).disable_test_eval
    assert driver.parse_args(BASE + ["--disable-test-eval"]).disable_test_eval          # an evaluation may: it only warns
    ok = driver.parse_args(BASE + ["--dataset-test", "TinyImagenet200", "--disable-test-eval", "--analysis", "SuperclassNBDT",
                                   "--superclass-wnids", ANIMAL, VEHICLE, "--exclude-labels", "0", "1"])
    assert ok.analysis == "SuperclassNBDT" and ok.superclass_wnids == [ANIMAL, VEHICLE] and ok.label_subset == "exclude_labels"
    assert driver.parse_args(BASE + ["--dataset-test", "CIFAR10"]).dataset_test == "CIFAR10"     # the same label set: allowed
    assert driver.parse_args(BASE + ["--probability-labels", "0.5"]).probability_labels == [0.5]


def test_synthetic_test_labels_are_a_function_of_seed_label_set_and_count():
    a, _ = driver.synthetic_test_labels(0, 200, 128)
    b, _ = driver.synthetic_test_labels(0, 200, 128)
    assert torch.equal(a, b) and a.dtype == torch.int64 and 0 <= int(a.min()) and 150 < int(a.max()) < 200
    assert not torch.equal(a, driver.synthetic_test_labels(1, 200, 128)[0])


# ------------------------------------------------------------------------------------------------ C-ABI
ENTRIES = (("nbdt_groups_create", 6), ("nbdt_groups_destroy", 1), ("nbdt_group_logits", 7),
           ("nbdt_group_logits_backward", 5), ("nbdt_superclass_accumulate", 14))


def test_header_ctypes_table_and_version_agree():
    lib = _C.lib()
    assert lib.nbdt_version() >= 131
    text = open(os.path.join(nbdt_path.ROOT, "include", "nbdt_hip.h")).read()
    assert "superclass evaluation (nbdt_version() >= 131)" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    exported = set(_C.exported_symbols())
    for name, n_args in ENTRIES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert m and len(m.group(1).split(",")) == n_args == len(_C.SIGNATURES[name][1]), name
        assert name in exported, name
    assert re.search(r"#define\s+NBDT_SUPER_MASKED\s+0\b", code) and re.search(r"#define\s+NBDT_SUPER_GROUP_MEAN\s+1\b", code)
    assert (_C.NBDT_SUPER_MASKED, _C.NBDT_SUPER_GROUP_MEAN) == (0, 1) == (R.MASKED, R.GROUP_MEAN)
    from nbdt import _build
    assert _build.FLAGS["superclass.hip"] == _build.FLAGS["rules.hip"] and "superclass.hip" in _build.sources()
    source = open(os.path.join(_build.CSRC, "superclass.hip")).read()
    assert not re.search(r"atomicAdd\s*\(\s*(\(float|&?\w*f\b)", source) and "unsafe-fp-atomics" not in source


def test_groups_create_refusals_need_no_gpu():
    lib = _C.lib()
    out = ctypes.c_void_p()
    i32 = lambda v: np.asarray(v, dtype=np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))  # noqa: E731
    def create(C, G, off, cls):  # noqa: E306
        rc = lib.nbdt_groups_create(0, C, G, i32(off), i32(cls), ctypes.byref(out))
        return rc, lib.nbdt_last_error().decode()
    rc, why = create(10, 2, [0, 3, 5], [1, 2, 1, 4, 5])
    assert rc == EINVAL and "group 0 lists class 1 twice" in why
    rc, why = create(10, 2, [0, 2, 4], [1, 2, 3, 10])
    assert rc == EINVAL and "class index 10, outside [0, 10)" in why
    rc, why = create(10, 2, [0, 2, 4], [1, 2, -1, 3])
    assert rc == EINVAL and "class index -1" in why
    assert create(10, 2, [1, 2, 4], [1, 2, 3, 4])[0] == EINVAL and create(10, 2, [0, 3, 2], [1, 2, 3])[0] == EINVAL
    assert create(0, 2, [0, 1, 2], [0, 0])[0] == EINVAL and create(10, 0, [0], [0])[0] == EINVAL
    assert lib.nbdt_groups_destroy(None) == 0
    with pytest.raises(_C.NBDTHipError, match="twice"):
        _C.GroupsHandle([[1, 1]], 4, 0)
