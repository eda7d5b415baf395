"""EfficientNet-B0 -- the pytorchcv ``efficientnet_b0`` factory the reference re-exports at
nbdt/models/__init__.py:3 (README.md:141-151 uses it for ImageNet NBDTs)."""
from nbdt.engine_effnet import EfficientNetEngine
from nbdt.models._hip_module import HipBackbone


def efficientnet_b0(num_classes=1000, pretrained=False, in_size=(224, 224), dropout_rate=0.2, device="cuda",
                    seed=0, stochastic_depth_prob=0.0, **kwargs):
    """stochastic_depth_prob: torchvision's ``StochasticDepth(p, mode="row")`` on the units with a skip connection
    (``EfficientNetEngine.set_stochastic_depth``); 0, the default, is pytorchcv's model, which has none."""
    if pretrained:
        raise NotImplementedError("pretrained checkpoints need network access; use load_state_dict")
    return HipBackbone(EfficientNetEngine(num_classes=num_classes, dropout_rate=dropout_rate, device=device,
                                          seed=seed, stochastic_depth_prob=stochastic_depth_prob))


efficientnet_b0.engine_cls = EfficientNetEngine      # what main.py asks which engine-level flags an --arch takes
