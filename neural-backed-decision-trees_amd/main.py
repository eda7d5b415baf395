#!/usr/bin/env python3
"""Training / evaluation driver with the reference's ``main.py`` command line.

Mirrors reference main.py:28-90 (flags), :164-188 (``--resume`` / ``--path-resume`` with checkpoints
``{"net", "acc", "epoch"}`` and ``module.`` prefix coercion), :191-210 (loss construction from
``--loss``, SGD momentum 0.9 wd 5e-4 (``--weight-decay``; the ImageNet recipe's is 1e-4), MultiStepLR at 3/7 and 5/7 of ``--epochs``), :218-308 (train /
test loops, best-accuracy checkpointing to ``./checkpoint/<generate_checkpoint_fname>.pth``), so the
recipes in the reference's ``scripts/*.sh`` keep their arguments.  What differs, and why:

* One process per GPU instead of ``DataParallel`` (launch with ``python -m torch.distributed.run
  --nproc-per-node N main.py ...``): each rank trains on its shard, gradients are all-reduced (RCCL).
* The step itself is the engine's fixed launch sequence: forward, fused tree-supervision loss
  (loss + dL/dlogits in one kernel), backward, fused SGD -- no autograd graph, no optimizer object.
* Datasets: torchvision is not available on the target image and the reference's dataset/transform
  layer is out of scope, so samples come from ``--data-file`` (a ``torch.save``d
  dict with ``train_x [N,3,H,W]`` uint8|float, ``train_y``, ``test_x``, ``test_y``; already
  normalised if float, scaled to [0,1] and normalised with the reference's CIFAR statistics if uint8)
  or from ``--synthetic N`` (CIFAR-shaped noise with a learnable class signal, for smoke runs).  ``--augment none``
  (the default) feeds them as they are, gathered on the host.  ``--augment reference`` is the reference's training
  transform -- ``RandomCrop(size, padding) -> RandomHorizontalFlip -> ToTensor -> Normalize`` with the statistics and
  padding of ``nbdt.data.DATASET_STATS`` (reference nbdt/data/cifar.py:11-21, nbdt/data/imagenet.py:37-48): both splits
  become ``nbdt.data.DeviceDataset``s held on the GPU, and one launch per step gathers, crops, flips and normalises the
  batch there (a uint8 file is normalised in the kernel, a float file or ``--synthetic`` is taken as normalised and
  padded with ``(0 - mean)/std``); evaluation is the plain gather + normalise.  ``Imagenet1000`` is refused there: its
  ``RandomResizedCrop`` is a different transform, ``--augment resized-crop``.  That one is the reference's ImageNet recipe
  (nbdt/data/imagenet.py:152-172) on ``nbdt.data.ResizedCropDataset``s: a uint8 ``--data-file`` of any fixed ``H x W`` (or
  uint8 ``--synthetic`` images of side ``--image-size``) stays on the GPU as bytes; training batches are
  ``RandomResizedCrop(S) -> RandomHorizontalFlip -> Normalize``, evaluation batches ``Resize(S + 32) -> CenterCrop(S) ->
  Normalize``, one launch each, resampled with PIL's bilinear filter.  ``S`` is 224 (``nbdt.data.RESIZED_CROP_STATS``)
  unless ``--crop-size`` says otherwise.
* ``--analysis Noop | SoftEmbeddedDecisionRules | HardEmbeddedDecisionRules`` drives an analyzer of ``nbdt.analysis``
  through the reference's hook protocol (reference main.py:212-288, nbdt/analysis.py:81-130): ``epoch_context`` around
  every epoch, ``start_train`` / ``end_train`` around the training pass, ``start_test`` / ``update_batch(logits,
  targets, images)`` per evaluation batch / ``end_test``.  The two rules analyzers report the accuracy of the decision
  rules applied to the backbone's logits (reference nbdt/analysis.py:204-252) next to the backbone's ``--metric``; their
  counters stay on the device, one host transfer per evaluation.  The training pass does not call ``update_batch``: the
  fused step (classifier + rules + loss + their backward in one launch) never materialises the logits.
* ``--diagnostics TreeStatistics ConfusionMatrix Entropy TopDifference NBDTEntropyMaxMin`` (any of them) runs the
  analyzers of ``nbdt.diagnostics`` beside the ``--analysis`` analyzer, in a ``diagnostics.Chain``: per-node accuracy and
  entropy, the depth of the first wrong turn, confusion matrices and entropy rankings from one fused launch per
  evaluation batch; ``--diagnostics-out FILE`` writes the last evaluation's report as JSON.
* ``--analysis Superclass | SuperclassNBDT --superclass-wnids W1 W2 ...`` is the reference's zero-shot evaluation on
  superclasses (``nbdt.superclass``, one launch per evaluation batch): ``--dataset-test D`` names the label set of the
  evaluation split, which comes from ``--data-file-test F`` (its ``test_x`` / ``test_y``) or, with ``--synthetic``, is a
  synthetic split with labels in ``[0, C_test)``; ``--disable-test-eval`` (required when the two label sets differ) skips
  the criterion and the backbone's hit counter, whose labels would index another label set; in a training run the best
  checkpoint is then kept by the analyzer's accuracy (its ``acc`` field holds that), so the run needs an ``--analysis``
  that reports one.  ``--superclass-file`` is an
  explicit hypernym table; without it and without nltk the mapping comes from the shipped WordNet graph, lossily.
* ``--include-labels`` / ``--exclude-labels`` / ``--probability-labels`` / ``--include-classes`` (reference
  nbdt/data/custom.py) restrict the TRAINING split: ``nbdt.data.label_subset`` picks the kept samples once, with the
  reference's draw, and every epoch's permutation is drawn over them (``nbdt.dist.epoch_indices(subset=)``) -- with the
  device-resident datasets too, and within each rank's range under ``--shard-data``.  Labels keep their numbering.
* Evaluation is distributed whenever there is more than one rank: rank r of w evaluates the samples
  ``nbdt.data.shard_range(N, r, w)`` of the test split, the hit counts and the loss are summed over ranks with one
  all-reduce, and every analyzer's ``reduce()`` merges the ranks' statistics, so what rank 0 prints, writes and
  checkpoints on is the whole split's, as in a one-rank run.
* ``--shard-data`` (with ``--augment reference | resized-crop``) keeps on each GPU only that rank's contiguous part of
  both splits (``shard=(rank, world)``: ImageNet at 256 x 256 is 252 GB whole, 31.5 GB per rank at 8 ranks); a
  ``--data-file`` is then memory-mapped, so a rank reads only its part of it.  Training shuffles WITHIN each rank's shard
  (``nbdt.dist.epoch_indices(..., sharded=True)``), not across the whole set as the reference's sampler does: a global
  batch is ``batch / world`` samples from every rank's part.  That is the price of never moving an image between GPUs;
  the augmentation a sample gets is the same either way (it depends on seed, epoch and the sample's index alone).
* ``--label-smoothing E`` wraps ``nn.CrossEntropyLoss(label_smoothing=E)``; the fused tree losses apply it in their one
  launch.  ``--mixup-alpha A`` / ``--cutmix-alpha A`` mix every training batch with itself rolled by one
  (torchvision v2's MixUp / CutMix, one draw per step: ``nbdt.data.draw_mix`` of (seed, epoch, step), the same on every
  rank) in one launch that also writes the probability targets, whatever ``--augment`` made the batch; the step then takes
  ``soft_target_loss_and_grad``.  A loss without it (``HardTreeSupLoss``: the reference's cannot take probability
  targets either) is refused at argument time.  Evaluation is never mixed.
* ``--auto-augment ta_wide`` applies TrivialAugmentWide (one of 14 operations at one of 31 magnitudes per image, Pillow's
  pixel rules) and ``--random-erase P`` torchvision's ``RandomErasing(P, value=0)`` to every training image, inside the
  one batch-assembly launch of ``--augment reference`` (``nbdt.data.DeviceDataset(policy=, erase_prob=)``,
  ``nbdt_policy_batch``): gather, padded crop, flip, the operation on the bytes, normalise, erase.  Both need a uint8
  ``--data-file``; ``--augment resized-crop`` does not have them in its one launch.  MixUp / CutMix still run on the
  assembled batch.
* ``--augment resized-crop-policy`` is ``resized-crop`` with them: ``--auto-augment ta_wide | ra | cifar10 | imagenet`` and
  ``--random-erase`` on the ``S x S`` crop (at most 512 x 512), between the flip and the normalisation and after it
  (``nbdt.data.ResizedCropDataset(policy=, erase_prob=)``, ``nbdt_resized_crop_policy_batch``: the resampling launch
  writes bytes, a second launch runs the chain between two global-memory tiles per image).  ``--crop-size``,
  ``--shard-data`` and the evaluation transform are ``resized-crop``'s; it needs a uint8 ``--data-file``.
* ``--auto-augment ra`` (RandAugment: ``--ra-num-ops`` N in 1..4 operations per image, each uniform among the 14, at bin
  ``--ra-magnitude`` M in 0..30 with a random sign) and ``--auto-augment cifar10`` (AutoAugment's CIFAR-10 policy: one of 25
  sub-policies of two (op, probability, magnitude) slots per image) run the whole chain in the same launch
  (``nbdt_policy_chain_batch``; ``DeviceDataset(policy="ra" | "cifar10")``), under the preconditions of ``ta_wide``.
* ``--optimizer lars`` replaces the SGD pass with layer-wise adaptive rate scaling (You et al. 2017; apex's
  ``LARC(clip=False)`` around ``optim.SGD``): ``engine.lars_step``, three launches over the flat parameter arena.
  ``--lars-trust`` / ``--lars-eps`` are its coefficients; BatchNorm parameters and biases take plain SGD steps without decay
  unless ``--lars-adapt-1d``.  ``--warmup-epochs W`` ramps the learning rate linearly over the first ``W`` epochs' steps and
  ``--lr-schedule cosine | poly`` decays it per step afterwards (Goyal et al. 2017; ``lr_at``): the large-batch recipe for a
  whole node, e.g. 8 ranks at ``--batch-size 4096``.  With the defaults (``sgd``, ``multistep``, no warm-up) the learning
  rate is the reference's MultiStepLR, evaluated once per epoch, and the step is the SGD step.
* ``--optimizer adamw | rmsprop`` make the optimizer pass ``engine.adamw_step`` (``torch.optim.AdamW``: ``--adam-betas``,
  ``--opt-eps``, ``--weight-decay`` decoupled) or ``engine.rmsprop_step`` (``torch.optim.RMSprop`` with the driver's momentum
  0.9, ``--rmsprop-alpha``, ``--opt-eps``; ``--rmsprop-tf`` is TensorFlow's form with its defaults alpha 0.9 and eps 1e-3, the
  one EfficientNet was trained with): one launch over the flat parameter arena and a second state arena
  (``ParamStore.sq``), BatchNorm parameters and biases undecayed unless ``--opt-decay-1d``.  ``--lr-schedule exp``
  multiplies the learning rate by ``--lr-decay-rate`` every ``--lr-decay-epochs`` epochs after the warm-up (0.97 every 2.4
  epochs: the EfficientNet recipe, with ``--ema-decay 0.9999``).  The checkpoint's name gains ``-adamw`` / ``-rmsprop``;
  like the reference's, a checkpoint holds no optimizer state.
* ``--ema-decay D`` keeps an exponential moving average of the weights and the BatchNorm running statistics inside the
  engine (``engine.ema_enable`` / ``ema_update``: two launches after every ``--ema-steps``-th optimizer step, with the
  usual ``(1 + t) / (10 + t)`` warm-up of the decay unless ``--no-ema-warmup``).  Every evaluation still reports the live
  weights exactly as before, then evaluates once more inside ``engine.ema_weights()`` and logs ``EMA Accuracy``; a saved
  checkpoint gains ``net_ema``, ``acc_ema`` and ``ema_updates`` and its name ``-ema``.  ``--resume`` restores the average
  when the checkpoint has one, else starts it from the loaded weights; ``--eval --resume --use-ema`` evaluates ``net_ema``.
  ``SoftTreeLoss`` keeps inducing hierarchies from the live classifier.  Every rank keeps its own, bit-identical, average.
* ``--stochastic-depth P`` (``--arch efficientnet_b0`` .. ``efficientnet_b7b``) is torchvision's
  ``StochasticDepth(p, mode="row")``: in training, image ``b`` of MBConv unit ``i`` of the architecture's ``U`` units (16 for
  B0, 55 for B7) loses its branch with probability ``P * i / U`` wherever the unit has a skip
  connection, inside the residual add and the BatchNorm backward that run anyway, plus one launch per forward that
  draws the factors (``engine.set_stochastic_depth(P, stream=rank)``: every rank and every micro-batch of
  ``--accum-steps`` draws its own).  Evaluation and ``--eval`` ignore it.  The draw's counter is not saved: a resumed run
  restarts it.
"""
import argparse
import json
import math
import os
import sys
from pathlib import Path

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nbdt import analysis  # noqa: E402
from nbdt import diagnostics  # noqa: E402
from nbdt import dist as ndist  # noqa: E402
from nbdt import loss as losses  # noqa: E402
from nbdt import models  # noqa: E402
from nbdt import superclass  # noqa: E402
from nbdt.data import (DATASET_STATS, RESIZED_CROP_STATS, DeviceDataset, ResizedCropDataset, draw_mix, label_subset,  # noqa: E402
                       mix_batch, shard_range)
from nbdt.engine import train_step  # noqa: E402
from nbdt.model import coerce_state_dict  # noqa: E402
from nbdt.tree import Tree, get_wnids  # noqa: E402
from nbdt.utils import DATASET_TO_NUM_CLASSES, DATASETS, SEGMENTATION_DATASETS, dataset_to_default_path_wnids  # noqa: E402

CIFAR_MEAN, CIFAR_STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)   # reference nbdt/data/cifar.py:17-19
METRICS = {"top1": 1, "top2": 2, "top5": 5, "top10": 10}      # the reference's --metric names -> k


class HitCounter:
    """Running count of samples whose target is among the k largest scores.  Both counters stay on the device;
    `percent()` is the only host transfer."""

    def __init__(self, k, device):
        self.k = k
        self.hits = torch.zeros((), dtype=torch.long, device=device)
        self.seen = 0

    def add(self, scores, targets):
        k = min(self.k, scores.shape[1])
        if k == 1:
            self.hits += (scores.argmax(dim=1) == targets).sum()
        else:
            self.hits += (scores.topk(k, dim=1).indices == targets[:, None]).any(dim=1).sum()
        self.seen += targets.shape[0]

    def percent(self):
        return 100.0 * int(self.hits) / max(self.seen, 1)


def build_parser():
    p = argparse.ArgumentParser(description="NBDT training on MI355X (reference main.py command line)")
    p.add_argument("--batch-size", default=512, type=int, help="GLOBAL batch size (split over ranks)")
    p.add_argument("--epochs", "-e", default=200, type=int, help="lr schedule is scaled accordingly")
    p.add_argument("--dataset", default="CIFAR10",
                   choices=[d for d in DATASETS if d not in SEGMENTATION_DATASETS])     # a classification driver
    p.add_argument("--arch", default="ResNet18", choices=models.get_model_choices())
    p.add_argument("--lr", default=0.1, type=float)
    p.add_argument("--weight-decay", default=5e-4, type=float, help="SGD weight decay (the reference's ImageNet recipe: 1e-4)")
    p.add_argument("--resume", "-r", action="store_true")
    p.add_argument("--path-resume", default="")
    p.add_argument("--name", default="")
    p.add_argument("--pretrained", action="store_true")
    p.add_argument("--eval", action="store_true")
    p.add_argument("--loss", choices=losses.names, default=["CrossEntropyLoss"], nargs="+")
    p.add_argument("--metric", choices=sorted(METRICS), default="top1")
    p.add_argument("--analysis", choices=analysis.names + superclass.names,
                   help="analyzer run during every evaluation (nbdt.analysis; Superclass / SuperclassNBDT: nbdt.superclass)")
    p.add_argument("--dataset-test", choices=[d for d in DATASETS if d not in SEGMENTATION_DATASETS],
                   help="the label set of the evaluation split (default: --dataset); another one needs --disable-test-eval")
    p.add_argument("--data-file-test", metavar="F",
                   help="with --dataset-test: torch.save'd dict whose test_x / test_y are the evaluation split")
    p.add_argument("--disable-test-eval", action="store_true",
                   help="evaluation skips the criterion and the backbone's hit counter (their labels would index another "
                        "label set); use --analysis to define the metric")
    superclass.add_arguments(p)     # --superclass-wnids / --superclass-file
    # label subsets of the training split (reference nbdt/data/custom.py:37-41)
    p.add_argument("--probability-labels", nargs="*", type=float, metavar="P",
                   help="keep a training sample of label c with probability P[c] (one value: every label)")
    p.add_argument("--include-labels", nargs="*", type=int, metavar="C", help="train on these labels only")
    p.add_argument("--exclude-labels", nargs="*", type=int, metavar="C", help="train on every label but these")
    p.add_argument("--include-classes", nargs="*", metavar="WNID",
                   help="--include-labels by name: the WordNet ids of the dataset's classes (nbdt/wnids/<dataset>.txt)")
    p.add_argument("--diagnostics", choices=diagnostics.names, nargs="+", default=[],
                   help="tree diagnostics run beside --analysis during every evaluation (nbdt.diagnostics)")
    p.add_argument("--diagnostics-out", metavar="FILE", help="write the diagnostics of the last evaluation as JSON")
    # nbdt/tree.py:26-35
    p.add_argument("--hierarchy")
    p.add_argument("--path-graph")
    p.add_argument("--path-wnids")
    p.add_argument("--induce-hierarchy", action="store_true",
                   help="with --resume --path-resume FILE: write the hierarchy induced-<arch> (or --path-graph) from that "
                        "checkpoint's classifier before the tree is built -- agglomerative clustering on the GPU "
                        "(csrc/linkage.hip) -- then go on as usual")
    p.add_argument("--induced-linkage", default="ward", choices=("ward", "complete", "single", "average"),
                   help="--induce-hierarchy: the linkage (ward is what every shipped hierarchy uses)")
    losses.add_arguments(p)     # --xent-weight* / --tree-supervision-weight* / --tree-*-epochs (reference nbdt/loss.py:27-80)
    # data source (see module docstring)
    p.add_argument("--data-file", help="torch.save'd dict: train_x, train_y, test_x, test_y")
    p.add_argument("--synthetic", type=int, default=0, help="number of synthetic training samples")
    p.add_argument("--image-size", type=int, default=0, help="synthetic image size (default: dataset's)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--augment", choices=("none", "reference", "resized-crop", "resized-crop-policy"), default="none",
                   help="reference: the reference's RandomCrop(padding) + RandomHorizontalFlip + Normalize on a "
                        "device-resident dataset, one launch per step (nbdt.data); resized-crop: its ImageNet recipe, "
                        "RandomResizedCrop + RandomHorizontalFlip + Normalize for training and Resize + CenterCrop for "
                        "evaluation, on a device-resident uint8 dataset; resized-crop-policy: resized-crop with "
                        "--auto-augment / --random-erase on the crop (a second launch per step); none: samples as they are")
    p.add_argument("--crop-size", type=int, default=0,
                   help="--augment resized-crop | resized-crop-policy: output side S (default: the dataset's, 224); evaluation "
                        "resizes to S + 32")
    p.add_argument("--shard-data", action="store_true",
                   help="--augment reference | resized-crop: every rank keeps only its contiguous part of both splits on "
                        "its GPU (nbdt.data shard=(rank, world)), a --data-file is memory-mapped, and training shuffles "
                        "within each rank's part")
    p.add_argument("--auto-augment", choices=("none", "ta_wide", "ra", "cifar10", "imagenet"), default="none",
                   help="ta_wide: TrivialAugmentWide, one of 14 operations at one of 31 magnitudes per training image; ra: "
                        "RandAugment, --ra-num-ops operations at magnitude --ra-magnitude; cifar10 / imagenet: AutoAugment's "
                        "CIFAR-10 / ImageNet policy (25 sub-policies of two operations).  Inside the batch-assembly launch "
                        "of --augment reference (nbdt.data DeviceDataset(policy=)), or on the crop of --augment "
                        "resized-crop-policy (ResizedCropDataset(policy=)); both on a uint8 --data-file")
    p.add_argument("--ra-num-ops", type=int, default=2, metavar="N", help="RandAugment: operations per image, 1..4")
    p.add_argument("--ra-magnitude", type=int, default=9, metavar="M", help="RandAugment: the magnitude bin, 0..30")
    p.add_argument("--random-erase", type=float, default=0.0, metavar="P",
                   help="torchvision's RandomErasing(P, value=0) on every training image after the normalisation, in the "
                        "same launch (--augment reference | resized-crop-policy on a uint8 --data-file); 0: off")
    p.add_argument("--label-smoothing", type=float, default=0.0, metavar="E",
                   help="label_smoothing of the wrapped nn.CrossEntropyLoss, 0 <= E < 1 (applied inside the fused tree loss)")
    p.add_argument("--mixup-alpha", type=float, default=0.0, metavar="A",
                   help="MixUp on every training batch, lam ~ Beta(A, A) per step (0: off); with --cutmix-alpha too, a fair "
                        "coin per step picks one of the two")
    p.add_argument("--cutmix-alpha", type=float, default=0.0, metavar="A",
                   help="CutMix on every training batch, lam ~ Beta(A, A) per step (0: off)")
    p.add_argument("--deterministic", action="store_true",
                   help="bit-reproducible training steps, like the reference's CPU path: every cross-block reduction in "
                        "a fixed order instead of fp32 atomics (nbdt_set_deterministic; ResNet / WideResNet backbones)")
    p.add_argument("--optimizer", choices=("sgd", "lars", "adamw", "rmsprop"), default="sgd",
                   help="lars: layer-wise adaptive rate scaling (engine.lars_step) for large global batches; adamw: "
                        "torch.optim.AdamW (engine.adamw_step), for fine-tuning; rmsprop: torch.optim.RMSprop or, with "
                        "--rmsprop-tf, TensorFlow's (engine.rmsprop_step), momentum 0.9")
    p.add_argument("--adam-betas", type=float, nargs=2, default=(0.9, 0.999), metavar=("B1", "B2"),
                   help="--optimizer adamw: decay rates of the two moment estimates")
    p.add_argument("--opt-eps", type=float, default=None, metavar="EPS",
                   help="--optimizer adamw | rmsprop: the denominator's epsilon (default 1e-8; 1e-3 with --rmsprop-tf)")
    p.add_argument("--rmsprop-alpha", type=float, default=None, metavar="A",
                   help="--optimizer rmsprop: decay of the mean square (default 0.99; 0.9 with --rmsprop-tf)")
    p.add_argument("--rmsprop-tf", action="store_true",
                   help="--optimizer rmsprop: TensorFlow's form (epsilon inside the root, the learning rate inside the "
                        "momentum buffer, the mean square started at 1): the one EfficientNet was trained with")
    p.add_argument("--opt-decay-1d", action="store_true",
                   help="--optimizer adamw | rmsprop: decay BatchNorm parameters and biases too (default: no decay on them)")
    p.add_argument("--lars-trust", type=float, default=1e-3, help="--optimizer lars: trust coefficient")
    p.add_argument("--lars-eps", type=float, default=1e-8, help="--optimizer lars: added to the trust ratio's denominator")
    p.add_argument("--lars-adapt-1d", action="store_true",
                   help="--optimizer lars: adapt and decay BatchNorm parameters and biases too (default: plain SGD, no decay)")
    p.add_argument("--lr-schedule", choices=("multistep", "cosine", "poly", "exp"), default="multistep",
                   help="multistep: the reference's MultiStepLR per epoch; cosine / poly: per-step decay to 0 after warm-up; "
                        "exp: times --lr-decay-rate every --lr-decay-epochs epochs after warm-up (the RMSprop recipe)")
    p.add_argument("--lr-decay-rate", type=float, default=0.97, metavar="G",
                   help="--lr-schedule exp: the factor of each decay, 0 < G <= 1")
    p.add_argument("--lr-decay-epochs", type=float, default=2.4, metavar="E",
                   help="--lr-schedule exp: epochs between two decays (may be fractional), > 0")
    p.add_argument("--warmup-epochs", type=float, default=0.0, metavar="W",
                   help="linear learning-rate warm-up over the first W epochs' steps (may be fractional)")
    p.add_argument("--ema-decay", type=float, default=None, metavar="D",
                   help="keep an exponential moving average of the weights with decay D, 0 < D < 1 (engine.ema_update), "
                        "evaluate it after the live weights and save it as net_ema (default: off)")
    p.add_argument("--ema-steps", type=int, default=1, metavar="K",
                   help="--ema-decay: update the average after every K-th optimizer step, with D as given")
    p.add_argument("--no-ema-warmup", action="store_true",
                   help="--ema-decay: decay D from the first update on, instead of min(D, (1 + t) / (10 + t))")
    p.add_argument("--use-ema", action="store_true",
                   help="--eval --resume: evaluate the checkpoint's averaged weights (net_ema) instead of net")
    p.add_argument("--accum-steps", type=int, default=1, metavar="K",
                   help="gradient accumulation: every rank runs its share of --batch-size (still the GLOBAL batch of one "
                        "optimizer step) as K micro-batches of batch / (ranks * K) images; one all-reduce and one "
                        "optimizer step per K (train_step micro_batches=K)")
    p.add_argument("--clip-grad-norm", type=float, default=None, metavar="M",
                   help="clip the gradient's global L2 norm to M before every optimizer step, on the device "
                        "(engine.clip_grad_norm; torchvision's --clip-grad-norm).  Default: off")
    p.add_argument("--stochastic-depth", type=float, default=0.0, metavar="P",
                   help="stochastic depth (drop-connect) on the MBConv units with a skip connection, torchvision's "
                        "StochasticDepth(P * i / units, 'row') for unit i, in training only (--arch efficientnet_b0 .. b7b; the "
                        "published recipe: 0.2).  Default 0: off")
    return p


def generate_checkpoint_fname(dataset, arch, path_graph=None, name="", tree_supervision_weight=1,
                              loss=("CrossEntropyLoss",), lr=0.1, tree_supervision_weight_end=None,
                              tree_supervision_weight_power=1, xent_weight=1, xent_weight_end=None,
                              xent_weight_power=1, **_):
    """reference nbdt/utils.py:266-330 (the parts reachable from this driver's flags)."""
    fname = f"ckpt-{dataset}-{arch}"
    if lr != 0.1:
        fname += f"-lr{lr}"
    if name:
        fname += "-" + name
    if path_graph and any("TreeSupLoss" in l for l in loss):   # (SoftTreeLoss does not match: reference quirk)
        fname += "-" + Path(path_graph).stem.replace("graph-", "", 1)
    if len(loss) > 1 or loss[0] != "CrossEntropyLoss":
        fname += f'-{",".join(loss)}'
        if tree_supervision_weight not in (None, 1):
            fname += f"-tsw{tree_supervision_weight}"
        if tree_supervision_weight_end not in (tree_supervision_weight, None):
            fname += f"-tswe{tree_supervision_weight_end}"
        if tree_supervision_weight_power not in (None, 1):
            fname += f"-tswp{tree_supervision_weight_power}"
        if xent_weight not in (None, 1):
            fname += f"-xw{xent_weight}"
        if xent_weight_end not in (xent_weight, None):
            fname += f"-xwe{xent_weight_end}"
        if xent_weight_power not in (None, 1):
            fname += f"-xwp{xent_weight_power}"
    return fname


def multistep_lr(base_lr, epoch, epochs, gamma=0.1):
    """optim.lr_scheduler.MultiStepLR(milestones=[int(3/7*E), int(5/7*E)]) -- reference main.py:208-210."""
    milestones = (int(3 / 7.0 * epochs), int(5 / 7.0 * epochs))
    return base_lr * gamma ** sum(epoch >= m for m in milestones)


def lr_at(base_lr, step, steps_per_epoch, epochs, schedule="multistep", warmup_epochs=0.0, decay_rate=0.97,
          decay_epochs=2.4):
    """Learning rate of global step `step` (0-based, `steps_per_epoch` per epoch).  T_w = round(W * steps_per_epoch)
    warm-up steps ramp linearly, base * (step + 1) / T_w (Goyal et al. 2017); then `multistep` is multistep_lr of the
    step's epoch, `cosine` is 0.5 * base * (1 + cos(pi * t)) and `poly` is base * (1 - t)^2 with
    t = (step - T_w) / (T - T_w), T = epochs * steps_per_epoch: both start at base on step T_w and would reach 0 on step
    T, one past the last step a run takes.  `exp` is base * decay_rate^floor((step - T_w) / S) with
    S = round(decay_epochs * steps_per_epoch) steps (at least 1): optim.lr_scheduler.StepLR(S, decay_rate) stepped once
    per optimizer step, the staircase of the RMSprop recipes (0.97 every 2.4 epochs)."""
    t_w = int(round(warmup_epochs * steps_per_epoch))
    total = epochs * steps_per_epoch
    if step < t_w:
        return base_lr * (step + 1) / t_w
    if schedule == "multistep":
        return multistep_lr(base_lr, step // steps_per_epoch, epochs)
    if schedule == "exp":
        every = max(int(round(decay_epochs * steps_per_epoch)), 1)
        return base_lr * decay_rate ** ((step - t_w) // every)
    t = (step - t_w) / float(max(total - t_w, 1))
    if schedule == "cosine":
        return 0.5 * base_lr * (1.0 + math.cos(math.pi * t))
    if schedule == "poly":
        return base_lr * (1.0 - t) ** 2
    raise ValueError(f"unknown learning-rate schedule {schedule!r}")


def eval_state_of(checkpoint, use_ema, path="the checkpoint"):
    """What --resume loads as the network's weights: the checkpoint itself, or with --use-ema its averaged weights."""
    if not use_ema:
        return checkpoint
    if "net_ema" not in checkpoint:
        raise SystemExit(f"--use-ema: {path} holds no averaged weights (no 'net_ema' key; it was not trained with "
                         "--ema-decay)")
    return {"net": checkpoint["net_ema"]}


def restore_ema(engine, checkpoint, reference_state_dict):
    """--resume with --ema-decay, after ema_enable started the average from the loaded weights: take the checkpoint's
    average and update count when it has them.  Returns whether it had."""
    if "net_ema" not in checkpoint:
        return False
    engine.load_ema_state_dict(coerce_state_dict({"net": checkpoint["net_ema"]}, reference_state_dict))
    engine.ema_updates = int(checkpoint.get("ema_updates", 0))
    return True


def ema_checkpoint_fields(engine, acc_ema):
    """The keys a checkpoint gains with --ema-decay."""
    return {"net_ema": {k: v.cpu() for k, v in engine.ema_state_dict().items()}, "acc_ema": acc_ema,
            "ema_updates": engine.ema_updates}


def build_criterion(args, tree, net=None, checkpoint_path="./"):
    """reference main.py:191-205: the LAST entry of --loss wraps nn.CrossEntropyLoss() (--label-smoothing: its
    label_smoothing)."""
    smoothing = float(getattr(args, "label_smoothing", 0.0))
    criterion = nn.CrossEntropyLoss(label_smoothing=smoothing)
    for name in args.loss:
        cls = getattr(losses, name)
        if name == "CrossEntropyLoss":
            criterion = cls(label_smoothing=smoothing)
            continue
        kwargs = {"dataset": args.dataset, "criterion": criterion, "tree": tree}
        for key in ("tree_supervision_weight", "tree_supervision_weight_end", "tree_supervision_weight_power",
                    "xent_weight", "xent_weight_end", "xent_weight_power"):
            if getattr(args, key) is not None:
                kwargs[key] = getattr(args, key)
        if name == "SoftTreeLoss":     # mid-training re-induction needs the network and a directory
            kwargs.update(net=net, arch=args.arch, checkpoint_path=checkpoint_path)
            for key in ("tree_start_epochs", "tree_update_every_epochs", "tree_update_end_epochs"):
                if getattr(args, key) is not None:
                    kwargs[key] = getattr(args, key)
        criterion = cls(**kwargs)
    return criterion


class _PlainCE:
    """--loss CrossEntropyLoss on the engine's fast path: the fused kernel with a zero tree weight."""

    def __init__(self, tree, label_smoothing=0.0):
        self.inner = losses.SoftTreeSupLoss(dataset=None, criterion=nn.CrossEntropyLoss(label_smoothing=label_smoothing),
                                            tree=tree, tree_supervision_weight=0.0)

    def set_epoch(self, cur, total):
        pass

    def loss_and_grad(self, z, y, grad_scale=1.0):
        return self.inner.loss_and_grad(z, y, grad_scale)

    def soft_target_loss_and_grad(self, z, target_probs, grad_scale=1.0):
        return self.inner.soft_target_loss_and_grad(z, target_probs, grad_scale)


def resized_crop_family(args):
    """--augment resized-crop or resized-crop-policy: ResizedCropDataset, --crop-size, the Resize + CenterCrop evaluation."""
    return args.augment in ("resized-crop", "resized-crop-policy")


def load_data(args, num_classes, device, raw=False):
    """train_x, train_y, test_x, test_y on the host.  raw: a uint8 --data-file stays uint8 (the augmentation kernel
    normalises it).  --shard-data memory-maps the file: the datasets slice their rank's part out of it, and only that part
    is ever read."""
    if args.data_file:
        blob = torch.load(args.data_file, map_location="cpu", mmap=True) if getattr(args, "shard_data", False) \
            else torch.load(args.data_file, map_location="cpu")
        out = []
        for split in ("train", "test"):
            x, y = blob[f"{split}_x"], blob[f"{split}_y"].long()
            if raw and x.dtype == torch.uint8:
                out += [x.contiguous(), y]
                continue
            if resized_crop_family(args):
                raise SystemExit(f"--augment {args.augment} resamples bytes: {split}_x of {args.data_file} must be uint8, "
                                 f"not {x.dtype}")
            if x.dtype == torch.uint8:
                x = x.float().div_(255.0)
                mean = torch.tensor(CIFAR_MEAN).view(1, 3, 1, 1)
                std = torch.tensor(CIFAR_STD).view(1, 3, 1, 1)
                x = (x - mean) / std
            out += [x.float().contiguous(), y]
        return out
    n = args.synthetic or 4 * args.batch_size
    size = args.image_size or (64 if args.dataset == "TinyImagenet200" else 224 if args.dataset == "Imagenet1000" else 32)
    g = torch.Generator().manual_seed(args.seed + 17)
    proto = torch.randn(num_classes, 3, size, size, generator=g)      # one pattern per class + noise

    def make(m):
        y = torch.randint(0, num_classes, (m,), generator=g)
        x = proto[y] + torch.randn(m, 3, size, size, generator=g)
        if resized_crop_family(args):            # the resized crop reads bytes: the same signal around mid-grey
            x = (128.0 + 40.0 * x).round_().clamp_(0, 255).to(torch.uint8)
        return x.contiguous(), y
    return [*make(n), *make(max(n // 4, args.batch_size))]


def synthetic_test_labels(seed, num_classes_test, count):
    """(labels, generator): the labels of the synthetic --dataset-test split, uniform in [0, num_classes_test), drawn first
    from a generator of their own so that they are a function of (seed, label set, count) alone."""
    g = torch.Generator().manual_seed(int(seed) + 29)
    return torch.randint(0, int(num_classes_test), (int(count),), generator=g), g


def load_test_data(args, num_classes_test, like_x, raw=False):
    """The evaluation split of --dataset-test on the host: test_x / test_y of --data-file-test, prepared as load_data
    prepares a split, or with --synthetic a synthetic split shaped like the training images (`like_x`, whose count the
    usual quarter is taken of) with labels in [0, num_classes_test)."""
    if args.data_file_test:
        blob = torch.load(args.data_file_test, map_location="cpu")
        x, y = blob["test_x"], blob["test_y"].long()
        if raw and x.dtype == torch.uint8:
            return x.contiguous(), y
        if resized_crop_family(args):
            raise SystemExit(f"--augment {args.augment} resamples bytes: test_x of {args.data_file_test} must be uint8, "
                             f"not {x.dtype}")
        if x.dtype == torch.uint8:
            # deliberate: whatever --dataset-test is, its images are normalised as load_data normalises the images the
            # model was trained on (the CIFAR statistics, on this host path), not with the test set's own statistics
            x = x.float().div_(255.0)
            x = (x - torch.tensor(CIFAR_MEAN).view(1, 3, 1, 1)) / torch.tensor(CIFAR_STD).view(1, 3, 1, 1)
        return x.float().contiguous(), y
    if not args.synthetic:
        raise SystemExit("--dataset-test needs its evaluation split: --data-file-test F (test_x, test_y), or --synthetic")
    m = max(like_x.shape[0] // 4, args.batch_size)
    y, g = synthetic_test_labels(args.seed, num_classes_test, m)
    proto = torch.randn(num_classes_test, *like_x.shape[1:], generator=g)
    x = proto[y] + torch.randn(m, *like_x.shape[1:], generator=g)
    if like_x.dtype == torch.uint8:
        x = (128.0 + 40.0 * x).round_().clamp_(0, 255).to(torch.uint8)
    return x.contiguous(), y


def training_subset(args, train_y, num_classes):
    """--include-labels / --exclude-labels / --probability-labels / --include-classes: the kept training samples as an
    ascending int64 index tensor (nbdt.data.label_subset, seeded with --seed), or None without such a flag."""
    if not args.label_subset:
        return None
    kwargs = {args.label_subset: getattr(args, args.label_subset)}
    if args.label_subset == "include_classes":
        kwargs["classes"] = get_wnids(args.path_wnids or dataset_to_default_path_wnids(args.dataset))
    try:
        return label_subset(train_y, num_classes, seed=args.seed, **kwargs)
    except ValueError as e:
        raise SystemExit(f"--{args.label_subset.replace('_', '-')}: {e}") from e


def build_diagnostic(name, tree):
    """One analyzer of nbdt.diagnostics on the run's hierarchy (ConfusionMatrix: the backbone's own predictions)."""
    cls = getattr(diagnostics, name)
    if name in ("TreeStatistics", "NBDTEntropyMaxMin"):
        return cls(tree=tree)
    return cls(tree.classes)


def evaluate_part(net, criterion_module, analyzer, k, x, y, batch, device, rank=0, world=1, plain_eval=True):
    """One rank's part of an evaluation, nothing exchanged: the samples ``shard_range(N, rank, world)`` of (x, y) in
    batches of `batch`; every batch's logits also go to the analyzer (update_batch).  Returns (HitCounter, loss sum as a
    device scalar, number of batches).  x is a device-resident dataset -- sharded (it must be this rank's shard) or whole
    -- or a host tensor.  plain_eval=False (--disable-test-eval): the criterion and the hit counter are skipped -- the
    labels belong to another label set than the logits' columns -- and only the analyzer sees the batches."""
    net.eval()
    plain = HitCounter(k, device)
    loss_sum = torch.zeros((), device=device)
    batches = 0
    on_device = isinstance(x, (DeviceDataset, ResizedCropDataset))
    lo, hi = shard_range(x.global_size if on_device else x.shape[0], rank, world)
    if on_device and x.sharded and tuple(x.shard_range) != (lo, hi):
        raise ValueError(f"rank {rank} of {world} evaluates [{lo}, {hi}), the dataset holds {tuple(x.shard_range)}")
    if hasattr(analyzer, "set_sample_offset"):
        analyzer.set_sample_offset(lo)
    with torch.no_grad():
        order = torch.arange(lo, hi, device=device) if on_device else None
        for i in range(0, hi - lo, batch):
            if order is not None:           # device-resident split: the evaluation transform, one launch per batch
                xb, yb = x.batch(order[i:i + batch], train=False)
            else:
                j = min(lo + i + batch, hi)
                xb, yb = x[lo + i:j].to(device), y[lo + i:j].to(device)
            z = net(xb)
            batches += 1
            if plain_eval:
                loss_sum += criterion_module(z, yb)
                plain.add(z, yb)
            analyzer.update_batch(z, yb, xb)
    return plain, loss_sum, batches


def evaluate(net, criterion_module, analyzer, k, x, y, batch, device, rank=0, world=1, group=None, plain_eval=True):
    """reference main.py:262-277: top-k accuracy of the backbone's logits and the mean loss over (x, y); every batch's
    logits also go to the analyzer (update_batch), which keeps its own statistic.  With world > 1 every rank evaluates its
    part (evaluate_part), hits / seen / loss sum / batch count are summed over ranks with ONE all-reduce and the analyzer
    is reduced (analyzer.reduce): every rank returns, and its analyzer holds, the numbers of the whole split."""
    plain, loss_sum, batches = evaluate_part(net, criterion_module, analyzer, k, x, y, batch, device, rank, world,
                                             plain_eval=plain_eval)
    if world > 1:
        # one fp64 vector: the counts are integers far below 2^53, so their sums are exact
        part = torch.tensor([0.0, 0.0, plain.seen, batches], dtype=torch.float64, device=device)
        part[0], part[1] = plain.hits, loss_sum
        hits, loss_sum, seen, batches = ndist.sum_over_ranks(part, group).tolist()
        plain.hits.fill_(int(hits))
        plain.seen, batches = int(seen), int(batches)
        analyzer.reduce(group)
    return plain.percent(), float(loss_sum) / max(batches, 1)


def parse_args(argv=None):
    """The command line, with the combinations no run can honour refused before anything is built."""
    parser = build_parser()
    args = parser.parse_args(argv)
    if "ConfusionMatrix" in args.diagnostics and not args.eval:
        parser.error("--diagnostics ConfusionMatrix needs --eval: like the reference's, the analyzer refuses a training "
                     "pass (its start_train raises NotImplementedError)")
    if args.diagnostics_out and not args.diagnostics:
        parser.error("--diagnostics-out needs --diagnostics")
    if args.dataset_test and args.dataset_test != args.dataset and not args.disable_test_eval:
        parser.error(f"--dataset-test {args.dataset_test} differs from --dataset {args.dataset}: the criterion and the "
                     "backbone's hit counter would index another label set; pass --disable-test-eval and an --analysis")
    if args.disable_test_eval and not args.eval and args.analysis in (None, "Noop"):
        parser.error("--disable-test-eval in a training run needs an --analysis that reports an accuracy: nothing else "
                     "evaluates the epochs, and the best checkpoint is kept by it")
    if args.data_file_test and not args.dataset_test:
        parser.error("--data-file-test holds the evaluation split of --dataset-test: it needs --dataset-test")
    if args.analysis in superclass.names and not args.superclass_wnids:
        parser.error(f"--analysis {args.analysis} needs --superclass-wnids")
    if (args.superclass_wnids or args.superclass_file) and args.analysis not in superclass.names:
        parser.error("--superclass-wnids / --superclass-file belong to --analysis Superclass | SuperclassNBDT")
    subsets = [f for f in ("probability_labels", "include_labels", "exclude_labels", "include_classes")
               if getattr(args, f) is not None]
    if len(subsets) > 1:
        parser.error("--probability-labels, --include-labels, --exclude-labels and --include-classes each select the "
                     f"training subset: pass one of them, not {len(subsets)}")
    if subsets and not getattr(args, subsets[0]):
        parser.error(f"--{subsets[0].replace('_', '-')} needs at least one value")
    args.label_subset = subsets[0] if subsets else None
    if args.shard_data and not (args.augment == "reference" or resized_crop_family(args)):
        parser.error("--shard-data shards the device-resident datasets: it needs --augment reference, resized-crop or "
                     "resized-crop-policy")
    if not 0.0 <= args.random_erase <= 1.0:
        parser.error(f"--random-erase must be in [0, 1], got {args.random_erase}")
    if not 1 <= args.ra_num_ops <= 4:
        parser.error(f"--ra-num-ops must be 1..4, got {args.ra_num_ops}")
    if not 0 <= args.ra_magnitude <= 30:
        parser.error(f"--ra-magnitude must be 0..30, got {args.ra_magnitude}")
    if args.auto_augment != "none" or args.random_erase > 0:
        if args.augment == "resized-crop":
            parser.error("--auto-augment / --random-erase on --augment resized-crop is not built into that launch: use "
                         "--augment resized-crop-policy, which runs the policy on the crop in a second launch")
        if args.augment not in ("reference", "resized-crop-policy") or not args.data_file:
            parser.error("--auto-augment / --random-erase work on the bytes of a device-resident dataset: they need "
                         "--augment reference or --augment resized-crop-policy, and a uint8 --data-file")
    if args.augment == "resized-crop-policy" and not args.data_file:
        parser.error("--augment resized-crop-policy applies --auto-augment / --random-erase to the bytes of a uint8 "
                     "--data-file: it needs one")
    if not 0.0 <= args.label_smoothing < 1.0:
        parser.error(f"--label-smoothing must be in [0, 1), got {args.label_smoothing}")
    if args.mixup_alpha < 0 or args.cutmix_alpha < 0:
        parser.error("--mixup-alpha and --cutmix-alpha must be >= 0")
    if args.warmup_epochs < 0 or args.warmup_epochs > args.epochs:
        parser.error(f"--warmup-epochs must be in [0, --epochs], got {args.warmup_epochs}")
    if args.lars_trust <= 0 or args.lars_eps < 0:
        parser.error("--lars-trust must be > 0 and --lars-eps >= 0")
    if args.rmsprop_tf and args.optimizer != "rmsprop":
        parser.error("--rmsprop-tf belongs to --optimizer rmsprop")
    if args.opt_eps is None:             # the defaults of torch.optim.AdamW / RMSprop, or of the TensorFlow recipe
        args.opt_eps = 1e-3 if args.rmsprop_tf else 1e-8
    if args.rmsprop_alpha is None:
        args.rmsprop_alpha = 0.9 if args.rmsprop_tf else 0.99
    args.adam_betas = tuple(args.adam_betas)
    if not all(0.0 <= b < 1.0 for b in args.adam_betas):
        parser.error(f"--adam-betas must be in [0, 1), got {args.adam_betas}")
    if not 0.0 <= args.rmsprop_alpha < 1.0:
        parser.error(f"--rmsprop-alpha must be in [0, 1), got {args.rmsprop_alpha}")
    if not args.opt_eps >= 0.0 or math.isinf(args.opt_eps):
        parser.error(f"--opt-eps must be finite and >= 0, got {args.opt_eps}")
    if not 0.0 < args.lr_decay_rate <= 1.0:
        parser.error(f"--lr-decay-rate must be in (0, 1], got {args.lr_decay_rate}")
    if not 0.0 < args.lr_decay_epochs < math.inf:
        parser.error(f"--lr-decay-epochs must be > 0, got {args.lr_decay_epochs}")
    if args.ema_decay is not None and not 0.0 < args.ema_decay < 1.0:
        parser.error(f"--ema-decay must be in (0, 1), got {args.ema_decay}")
    if args.ema_steps < 1:
        parser.error(f"--ema-steps must be >= 1, got {args.ema_steps}")
    if args.accum_steps < 1:
        parser.error(f"--accum-steps must be >= 1, got {args.accum_steps}")
    if args.clip_grad_norm is not None and not 0.0 < args.clip_grad_norm < math.inf:
        parser.error(f"--clip-grad-norm must be finite and > 0, got {args.clip_grad_norm}")
    if not 0.0 <= args.stochastic_depth < 1.0:
        parser.error(f"--stochastic-depth must be in [0, 1), got {args.stochastic_depth}")
    if args.stochastic_depth > 0 and not hasattr(getattr(getattr(models, args.arch), "engine_cls", None),
                                                 "set_stochastic_depth"):
        parser.error(f"--stochastic-depth is built into the MBConv residual passes: --arch {args.arch} has no "
                     "set_stochastic_depth (the ResNet / WideResNet residual add lives inside conv epilogues); use "
                     "--arch efficientnet_b0 .. efficientnet_b7b")
    if args.use_ema and not (args.eval and args.resume):
        parser.error("--use-ema evaluates a checkpoint's averaged weights: it needs --eval and --resume")
    if args.induce_hierarchy:
        if not (args.resume and args.path_resume):
            parser.error("--induce-hierarchy clusters a trained classifier: it needs --resume --path-resume FILE")
        if args.hierarchy and args.hierarchy != f"induced-{args.arch}":
            parser.error(f"--induce-hierarchy writes induced-{args.arch} (or --path-graph), not --hierarchy {args.hierarchy}")
    if args.mixup_alpha > 0 or args.cutmix_alpha > 0:
        name = args.loss[-1]            # the loss the training step calls
        if name != "CrossEntropyLoss" and not hasattr(getattr(losses, name), "soft_target_loss_and_grad"):
            raise SystemExit(f"--mixup-alpha / --cutmix-alpha make probability targets, which --loss {name} cannot take "
                             f"(it has no soft_target_loss_and_grad; the reference's {name} cannot either): use "
                             "SoftTreeSupLoss, SoftTreeLoss or CrossEntropyLoss")
    return args


def induce_hierarchy(args, rank, world, log):
    """--induce-hierarchy: the step the README's "resolves only after generate_hierarchy(...)" asks for, in the run
    itself.  Rank 0 clusters the checkpoint's classifier rows on its GPU and writes the file (atomically), the others
    wait for it."""
    from nbdt.hierarchy import generate_hierarchy
    if not os.path.exists(args.path_resume):
        raise SystemExit(f"--induce-hierarchy: no checkpoint at {args.path_resume}")
    if rank == 0:
        path = generate_hierarchy(args.dataset, "induced", arch=args.arch, checkpoint=args.path_resume,
                                  induced_linkage=args.induced_linkage, path=args.path_graph or "",
                                  fname=f"graph-induced-{args.arch}", path_wnids=args.path_wnids,
                                  induced_backend="device")
        log(f"==> --induce-hierarchy: {path} from the classifier of {args.path_resume}")
    if world > 1:
        torch.distributed.barrier()
    if not args.path_graph:
        args.hierarchy = f"induced-{args.arch}"


def main(argv=None):
    args = parse_args(argv)
    if args.augment == "reference" and args.dataset not in DATASET_STATS:
        raise SystemExit(f"--augment reference: {args.dataset} trains with RandomResizedCrop in the reference, a different "
                         f"transform (--augment resized-crop); supported: {', '.join(sorted(DATASET_STATS))}")
    if resized_crop_family(args) and args.dataset not in RESIZED_CROP_STATS:
        raise SystemExit(f"--augment {args.augment}: {args.dataset} trains with RandomCrop(padding) in the reference "
                         f"(--augment reference); supported: {', '.join(sorted(RESIZED_CROP_STATS))}")
    if args.crop_size and not resized_crop_family(args):
        raise SystemExit("--crop-size belongs to --augment resized-crop | resized-crop-policy")
    on_device = args.augment == "reference" or resized_crop_family(args)      # both splits are datasets held on the GPU
    rank, world, local = ndist.init_from_env()
    if not torch.cuda.is_available():
        raise SystemExit("main.py needs an MI355X: the NBDT hot path has no CPU fallback")
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    log = print if rank == 0 else (lambda *a, **k: None)
    if args.pretrained:
        raise SystemExit("--pretrained downloads release checkpoints; load a local file with --resume --path-resume")
    if args.batch_size % world:
        raise SystemExit(f"--batch-size {args.batch_size} must be divisible by the number of ranks ({world})")
    if args.batch_size % (world * args.accum_steps):
        raise SystemExit(f"--batch-size {args.batch_size} must be divisible by ranks x --accum-steps "
                         f"({world} x {args.accum_steps})")

    num_classes = DATASET_TO_NUM_CLASSES[args.dataset]
    log("==> Preparing data..")
    train_x, train_y, test_x, test_y = load_data(args, num_classes, device, raw=on_device)
    if args.dataset_test and (args.dataset_test != args.dataset or args.data_file_test):
        # the evaluation split carries the labels of another label set (or is another file of the same one)
        test_x, test_y = load_test_data(args, DATASET_TO_NUM_CLASSES[args.dataset_test], train_x, raw=on_device)
    kept = training_subset(args, train_y, num_classes)     # before the labels move to the device: a host pass over them
    shard = (rank, world) if args.shard_data else None         # each rank keeps its contiguous part of both splits
    if args.augment == "reference":
        stats = DATASET_STATS[args.dataset]
        kwargs = dict(flip=True, device=device, shard=shard)
        policy = None if args.auto_augment == "none" else args.auto_augment
        if (policy or args.random_erase > 0) and train_x.dtype != torch.uint8:
            raise SystemExit(f"--auto-augment / --random-erase work on bytes: train_x of {args.data_file} must be uint8, "
                             f"not {train_x.dtype}")
        try:           # only the training split is augmented; evaluation never applies a policy
            train_x = DeviceDataset(train_x, train_y, stats["mean"], stats["std"], stats["pad"], policy=policy,
                                    erase_prob=args.random_erase, policy_ops=args.ra_num_ops,
                                    policy_magnitude=args.ra_magnitude, **kwargs)
        except ValueError as e:
            if policy or args.random_erase > 0:        # e.g. images too large for the policy kernel
                raise SystemExit(f"--auto-augment / --random-erase: {e}") from e
            raise
        if train_x.chain:
            log("--auto-augment " + (f"ra: RandAugment, {args.ra_num_ops} operations at magnitude {args.ra_magnitude}"
                                     if policy == "ra" else
                                     f"{policy}: AutoAugment, {len(train_x._subpolicies)} sub-policies")
                + " per training image, in the batch-assembly launch (nbdt_policy_chain_batch)")
        test_x = DeviceDataset(test_x, test_y, stats["mean"], stats["std"], stats["pad"], **kwargs)
    elif resized_crop_family(args):
        stats = RESIZED_CROP_STATS[args.dataset]
        size = args.crop_size or stats["size"]
        resize = size + 32 if args.crop_size else stats["resize"]       # reference: Resize(input_size + 32)
        kwargs = dict(size=size, resize=resize, scale=stats["scale"], ratio=stats["ratio"], flip=True, device=device,
                      shard=shard)
        policy = None if args.auto_augment == "none" else args.auto_augment        # (resized-crop-policy only: parse_args)
        try:           # only the training split is augmented; evaluation never applies a policy
            train_x = ResizedCropDataset(train_x, train_y, stats["mean"], stats["std"], policy=policy,
                                         erase_prob=args.random_erase, policy_ops=args.ra_num_ops,
                                         policy_magnitude=args.ra_magnitude, **kwargs)
        except ValueError as e:
            if policy or args.random_erase > 0:        # e.g. a crop too large for the policy kernel
                raise SystemExit(f"--auto-augment / --random-erase: {e}") from e
            raise
        if policy or args.random_erase > 0:
            what = {"ta_wide": "ta_wide: TrivialAugmentWide, one operation",
                    "ra": f"ra: RandAugment, {args.ra_num_ops} operations at magnitude {args.ra_magnitude}",
                    None: "none: no operation"}.get(policy) or \
                f"{policy}: AutoAugment, {len(train_x._subpolicies)} sub-policies"
            log(f"--auto-augment {what} per training image, --random-erase {args.random_erase:g}, on the {size} x {size} "
                "crop (nbdt_resized_crop_policy_batch)")
        test_x = ResizedCropDataset(test_x, test_y, stats["mean"], stats["std"], **kwargs)
    n_train = train_x.global_size if on_device else train_x.shape[0]
    n_test = test_x.global_size if on_device else test_x.shape[0]
    log(f"Training with dataset {args.dataset} and {num_classes} classes: {n_train} train / "
        f"{n_test} test samples of shape {tuple(train_x.shape[1:])}")
    if args.dataset_test:
        log(f"Testing with dataset {args.dataset_test} and {DATASET_TO_NUM_CLASSES[args.dataset_test]} classes")
    if kept is not None:
        log(f"--{args.label_subset.replace('_', '-')}: training on {kept.numel()} of the {n_train} training samples")
    if args.disable_test_eval and args.analysis in (None, "Noop"):
        log(" * Warning: --disable-test-eval without an --analysis: nothing measures the evaluation pass")
    if shard is not None:
        log(f"--shard-data: rank {rank} of {world} holds train samples {tuple(train_x.shard_range)} and test samples "
            f"{tuple(test_x.shard_range)}")

    log("==> Building model..")
    if args.deterministic:
        from nbdt import ops
        ops.set_deterministic(True)
    net = getattr(models, args.arch)(num_classes=num_classes, device=device, seed=args.seed)
    engine = net.engine
    if args.stochastic_depth > 0 and not args.eval:      # every rank drops its own images; evaluation never drops any
        engine.set_stochastic_depth(args.stochastic_depth, stream=rank)

    if not args.hierarchy and not args.path_graph and any("Tree" in l for l in args.loss) or args.analysis or args.diagnostics:
        args.hierarchy = args.hierarchy or f"induced-{args.arch}"       # reference nbdt/model.py:296-298 default
    if args.induce_hierarchy:
        induce_hierarchy(args, rank, world, log)
    tree = Tree.create_from_args(args)
    ck_args = dict(vars(args))
    ck_args["path_graph"] = tree.path_graph
    checkpoint_fname = generate_checkpoint_fname(**ck_args)
    if args.optimizer != "sgd":
        checkpoint_fname += "-" + args.optimizer
    if args.accum_steps > 1:
        checkpoint_fname += f"-acc{args.accum_steps}"
    if args.clip_grad_norm is not None:
        checkpoint_fname += f"-clip{args.clip_grad_norm}"
    ema_on = args.ema_decay is not None
    if ema_on or args.use_ema:
        checkpoint_fname += "-ema"
    checkpoint_path = f"./checkpoint/{checkpoint_fname}.pth"
    log(f"==> Checkpoints will be saved to: {checkpoint_path}")

    best_acc, start_epoch = 0.0, 0
    resume_path = args.path_resume or checkpoint_path
    if args.resume:
        log("==> Resuming from checkpoint..")
        if not os.path.exists(resume_path):
            if args.use_ema:
                raise SystemExit(f"--use-ema: no checkpoint at {resume_path} to take the averaged weights from")
            log("==> No checkpoint found. Skipping...")
        else:
            checkpoint = torch.load(resume_path, map_location="cpu")
            # {"net": ...} and `module.` prefix; --use-ema: the averaged weights are the ones to evaluate
            state = coerce_state_dict(eval_state_of(checkpoint, args.use_ema, resume_path), net.state_dict())
            net.load_state_dict(state)
            net._sync_mirrors()          # the engine reads the bf16 mirror / dgrad copies: refresh them now
            if "net" in checkpoint:
                best_acc, start_epoch = checkpoint["acc"], checkpoint["epoch"]
                log(f"==> Checkpoint found for epoch {start_epoch} with accuracy {best_acc} at {resume_path}")
            else:
                log(f"==> Checkpoint found at {resume_path}")
            if ema_on:                   # the average starts from the loaded weights unless the checkpoint brings its own
                engine.ema_enable(args.ema_decay, warmup=not args.no_ema_warmup)
                if restore_ema(engine, checkpoint, net.state_dict()):
                    log(f"==> Averaged weights restored after {engine.ema_updates} updates")
    if ema_on and engine.store.ema is None:
        engine.ema_enable(args.ema_decay, warmup=not args.no_ema_warmup)
    ema_analyzer = analysis.Noop(tree.classes)      # the averaged pass reports accuracy only; --analysis sees the live weights

    criterion = build_criterion(args, tree, net=net, checkpoint_path=checkpoint_path)
    fast = criterion if hasattr(criterion, "loss_and_grad") else _PlainCE(tree, args.label_smoothing)
    if args.analysis in superclass.names:
        try:
            analyzer = getattr(superclass, args.analysis)(tree=tree, superclass_wnids=args.superclass_wnids,
                                                          dataset_test=args.dataset_test, metric=args.metric,
                                                          hypernyms=args.superclass_file)
        except (ValueError, KeyError, RuntimeError) as e:
            raise SystemExit(f"--analysis {args.analysis}: {e}") from e
        log(f"==> Mapped {len(analyzer.mapped_classes)} of the {len(analyzer.wnids_test)} {analyzer.dataset_test} classes "
            f"to your superclasses; {[len(g) for g in analyzer.groups]} {args.dataset} classes under each")
    else:
        analyzer_cls = getattr(analysis, args.analysis or "Noop")
        analyzer = analyzer_cls(tree=tree, metric=args.metric) if args.analysis not in (None, "Noop") \
            else analyzer_cls(tree.classes)
    extras = [build_diagnostic(name, tree) for name in args.diagnostics]
    if extras:                                    # every rank ends up with the reduced statistic: rank 0 reports
        analyzer = diagnostics.Chain(analyzer, *extras)
    analyzer.verbose = rank == 0                  # one rank prints
    comm = ndist.GradComm() if world > 1 else None
    per_rank = args.batch_size // world
    # --weight-decay: handed on only when it is not train_step's own default
    decay = {} if args.weight_decay == 5e-4 else {"weight_decay": args.weight_decay}
    if args.optimizer == "lars":
        from nbdt.engine import LarsConfig
        decay["lars"] = LarsConfig(args.lars_trust, args.lars_eps, not args.lars_adapt_1d)
    elif args.optimizer == "adamw":
        from nbdt.engine import AdamWConfig
        decay["optim"] = AdamWConfig(args.adam_betas, args.opt_eps, not args.opt_decay_1d)
    elif args.optimizer == "rmsprop":
        from nbdt.engine import RMSpropConfig
        decay["optim"] = RMSpropConfig(args.rmsprop_alpha, args.opt_eps, args.rmsprop_tf, not args.opt_decay_1d)
    if args.accum_steps > 1:          # the mixed batch of a rank is cut into micro-batches inside train_step
        decay["micro_batches"] = args.accum_steps
    if args.clip_grad_norm is not None:
        from nbdt.engine import ClipConfig
        decay["clip"] = ClipConfig(args.clip_grad_norm)
    per_step_lr = args.lr_schedule != "multistep" or args.warmup_epochs > 0

    @analyzer.train_function
    def train(epoch):
        if hasattr(criterion, "set_epoch"):
            criterion.set_epoch(epoch, args.epochs)
        lr = multistep_lr(args.lr, epoch, args.epochs)
        # unsharded: the same shuffle of the whole set on every rank, each takes its slice of every global batch;
        # --shard-data: every rank shuffles the part it holds
        plan = ndist.epoch_indices(n_train, args.batch_size, rank, world, args.seed, epoch,
                                   sharded=shard is not None, subset=kept)
        steps = plan.shape[0]
        lrs = None
        if per_step_lr:          # warm-up / per-step decay: one learning rate per step of this epoch
            lrs = [lr_at(args.lr, epoch * steps + i, steps, args.epochs, args.lr_schedule, args.warmup_epochs,
                         args.lr_decay_rate, args.lr_decay_epochs) for i in range(steps)]
        if lrs and lrs[0] != lrs[-1]:
            log("\nEpoch: %d / LR: %.6f -> %.6f" % (epoch, lrs[0], lrs[-1]))
        else:
            log("\nEpoch: %d / LR: %.04f" % (epoch, lrs[0] if lrs else lr))
        net.train()
        total = torch.zeros((), device=device)
        if on_device:
            plan = plan.to(device)           # once per epoch; every step takes a row of it there
        for i in range(steps):
            idx = plan[i]
            if on_device:
                xb, yb = train_x.batch(idx, epoch=epoch, seed=args.seed)
            else:
                xb, yb = train_x[idx].to(device, non_blocking=True), train_y[idx].to(device, non_blocking=True)
            mix = draw_mix(args.seed, epoch, i, xb.shape[2], xb.shape[3], args.mixup_alpha, args.cutmix_alpha)
            if mix is not None:              # one launch: the mixed batch and its probability targets
                xb, yb = mix_batch(xb, yb, num_classes, mix)
            total += train_step(engine, fast, xb, yb, lrs[i] if lrs else lr, comm=comm, **decay)
            if ema_on and (epoch * steps + i + 1) % args.ema_steps == 0:
                engine.ema_update()          # two launches; every rank averages its own (bit-identical) replica
        log("Loss: %.3f (%d steps of %d x %d images)" % (total.item() / max(steps, 1), steps, world, per_rank))
        if args.clip_grad_norm is not None and rank == 0 and steps:      # one read-back per epoch, none per step
            c = engine.clip_stats()
            log("Clip: last norm %.4g, clipped %d of %d steps (max norm %g), %d non-finite"
                % (c["norm"], c["total_clipped"], c["steps"], args.clip_grad_norm, c["nonfinite"]))

    def test(epoch, checkpoint=True):
        nonlocal best_acc
        analyzer.start_test(epoch)
        acc, loss = evaluate(net, criterion, analyzer, METRICS[args.metric], test_x, test_y, 100, device, rank=rank,
                             world=world, plain_eval=not args.disable_test_eval)
        nbdt_acc = analyzer.accuracy() if hasattr(analyzer, "accuracy") else None
        extra = f" | {analyzer.name}: {nbdt_acc:.3f}%" if nbdt_acc is not None else ""
        if args.disable_test_eval:
            log("Loss and Acc not evaluated (--disable-test-eval)" + extra)
        else:
            log("Loss: %.3f | Acc: %.3f%%%s" % (loss, acc, extra))
        analyzer.end_test(epoch)
        # what "best" is measured by: the backbone's accuracy, or with --disable-test-eval (nothing evaluated the backbone)
        # the analyzer's -- parse_args refuses a training run that would have neither
        score = nbdt_acc if args.disable_test_eval and nbdt_acc is not None else acc
        log(f"Accuracy: {score} | Best Accuracy: {best_acc}" + (f" ({analyzer.name})" if score is not acc else ""))
        acc_ema = None
        if ema_on:       # every rank swaps: the evaluation is distributed.  Swapped back before anything is saved
            with engine.ema_weights():
                acc_ema, loss_ema = evaluate(net, criterion, ema_analyzer, METRICS[args.metric], test_x, test_y, 100,
                                             device, rank=rank, world=world, plain_eval=not args.disable_test_eval)
            log(f"EMA Accuracy: {acc_ema} | EMA Loss: {loss_ema:.3f} | {engine.ema_updates} updates")
        if score > best_acc and checkpoint and rank == 0:
            log(f"Saving to {checkpoint_fname} ({score})..")
            os.makedirs("checkpoint", exist_ok=True)
            blob = {"net": {k: v.cpu() for k, v in net.state_dict().items()}, "acc": score, "epoch": epoch}
            if ema_on:
                blob.update(ema_checkpoint_fields(engine, acc_ema))
            torch.save(blob, checkpoint_path)
        best_acc = max(best_acc, score)
        if extras and args.diagnostics_out and rank == 0:
            with open(args.diagnostics_out, "w") as f:
                json.dump({a.name: a.report() for a in extras}, f, indent=1)
        return acc, nbdt_acc

    if args.eval:
        if not args.resume:
            log(" * Warning: Model is not loaded from checkpoint. Use --resume")
        with analyzer.epoch_context(0):
            return test(0, checkpoint=False)
    result = None
    for epoch in range(start_epoch, args.epochs):
        with analyzer.epoch_context(epoch):
            train(epoch)
            result = test(epoch)
    return result


if __name__ == "__main__":
    main()
