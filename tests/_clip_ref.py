"""numpy restatement of nbdt_clip_norm / nbdt_clip_apply (include/nbdt_hip.h, "gradient clipping"): one array operation
per rounding.  The fp64 sum takes numpy's own order, not the kernel's partition: on fixtures whose sums are exact the
order does not matter, on random data the tests allow the one fp32 ulp the header's error argument gives."""
import numpy as np

EPS = np.float32(1e-6)


def new_record():
    """What a new plan's record holds."""
    return {"norm": np.float32(0.0), "coef": np.float32(1.0), "clipped": 0, "steps": 0, "nonfinite": 0, "total_clipped": 0}


def sum_of_squares(g):
    d = np.asarray(g, dtype=np.float32).ravel().astype(np.float64)
    with np.errstate(all="ignore"):
        return np.sum(d * d, dtype=np.float64)            # each product exact in fp64


def norm_of(g, grad_scale=1.0):
    """norm = fabsf(grad_scale) * sqrtf((float)S): the cast, the root, the multiply."""
    with np.errstate(all="ignore"):
        s32 = np.float32(sum_of_squares(g))
        r = np.sqrt(s32)
        assert r.dtype == np.float32
        return np.abs(np.float32(grad_scale)) * r


def fold(norm, max_norm, record):
    """From the fp32 norm: den, coef and the record's update.  Returns the coefficient nbdt_clip_apply will read."""
    norm = np.float32(norm)
    with np.errstate(all="ignore"):
        den = norm + EPS
        coef = np.float32(max_norm) / den
    assert den.dtype == np.float32 and coef.dtype == np.float32
    record["steps"] += 1
    record["clipped"] = 0
    if not np.isfinite(norm):
        coef = np.float32(1.0)
        record["nonfinite"] += 1
    elif coef < np.float32(1.0):
        record["clipped"] = 1
        record["total_clipped"] += 1
    else:
        coef = np.float32(1.0)
    record["norm"], record["coef"] = norm, coef
    return coef


def apply(g, coef):
    """g * coef, one fp32 multiply per element; coef == 1: g itself, untouched."""
    g = np.asarray(g, dtype=np.float32)
    if np.float32(coef) == np.float32(1.0):
        return g.copy()
    out = g * np.float32(coef)
    assert out.dtype == np.float32
    return out


def clip(g, grad_scale, max_norm, record=None):
    """The whole step: (clipped g, record)."""
    record = new_record() if record is None else record
    coef = fold(norm_of(g, grad_scale), max_norm, record)
    return apply(g, coef), record


def ulp_distance(a, b):
    """Number of fp32 values between two finite floats of one sign (0: the same bits)."""
    ia = int(np.float32(a).view(np.int32))
    ib = int(np.float32(b).view(np.int32))
    return abs(ia - ib)


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)
