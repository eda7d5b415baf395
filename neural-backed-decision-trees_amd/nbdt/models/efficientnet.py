"""EfficientNet-B0 .. B7 and their TF-padded `b` twins -- the pytorchcv ``efficientnet_b0`` .. ``efficientnet_b7b``
factories the reference re-exports at nbdt/models/__init__.py:3 (README.md:141-151 uses them for ImageNet NBDTs and
derives the ImageNet hierarchy from ``efficientnet_b7b``).  One engine, scaled by
``nbdt.engine_effnet.efficientnet_config``."""
from nbdt.engine_effnet import EFFNET_SCALING, EfficientNetEngine, efficientnet_config
from nbdt.models._hip_module import HipBackbone


def _factory(version, tf_mode):
    config = efficientnet_config(version, tf_mode)
    side = config["in_size"]
    name = f"efficientnet_{version}{'b' if tf_mode else ''}"

    def factory(num_classes=1000, pretrained=False, in_size=(side, side), dropout_rate=config["dropout_rate"],
                device="cuda", seed=0, stochastic_depth_prob=0.0, **kwargs):
        if pretrained:
            raise NotImplementedError("pretrained checkpoints need network access; use load_state_dict")
        return HipBackbone(EfficientNetEngine.from_config(config, num_classes=num_classes, dropout_rate=dropout_rate,
                                                          device=device, seed=seed,
                                                          stochastic_depth_prob=stochastic_depth_prob))

    factory.__name__ = factory.__qualname__ = name
    factory.__doc__ = (
        f"pytorchcv's ``{name}``: native input {side} x {side} (in_size is informational: the engine follows the batch "
        f"it is given, any side >= 32), dropout {config['dropout_rate']}"
        + (", TF \"SAME\" padding and BatchNorm eps 1e-3" if tf_mode else "") + ".\n"
        "stochastic_depth_prob: torchvision's ``StochasticDepth(p, mode=\"row\")`` on the units with a skip connection\n"
        "(``EfficientNetEngine.set_stochastic_depth``); 0, the default, is pytorchcv's model, which has none.")
    factory.engine_cls = EfficientNetEngine      # what main.py asks which engine-level flags an --arch takes
    factory.config = config
    return factory


EFFICIENTNET_NAMES = tuple(f"efficientnet_{v}{s}" for s in ("", "b") for v in sorted(EFFNET_SCALING))
for _v in EFFNET_SCALING:
    globals()[f"efficientnet_{_v}"] = _factory(_v, False)
    globals()[f"efficientnet_{_v}b"] = _factory(_v, True)
del _v
