"""The phantom the bias-field tests share: an ellipsoidal head of three tissues with a fine texture, a smooth multiplicative field on
the source side, and the two error figures the tests bound."""
import numpy as np

SHAPE = (40, 48, 36)


def phantom(shape=SHAPE):
    """-> (src, ref, field, src_mask, ref_mask): float32 volumes, ``src = ref * field``, uint8 masks ``> 100`` of each side."""
    g0, g1, g2 = np.meshgrid(*(np.linspace(-1.0, 1.0, n) for n in shape), indexing="ij")
    r = np.sqrt((g0 / 0.8) ** 2 + (g1 / 0.85) ** 2 + (g2 / 0.75) ** 2)
    tissue = (0.6 * (r < 0.9) + 0.25 * (r < 0.6) - 0.5 * (r < 0.25)) * (1.0 + 0.15 * np.sin(9.0 * g0) * np.cos(7.0 * g1))
    ref = 1000.0 * tissue
    field = np.exp(0.25 * g0 - 0.2 * g1 ** 2 + 0.15 * g2 * g0 + 0.1)
    src = ref * field
    src, ref, field = (np.ascontiguousarray(a, dtype=np.float32) for a in (src, ref, field))
    return src, ref, field, (src > 100).astype(np.uint8), (ref > 100).astype(np.uint8)


def relative_rms(a, b, inside):
    """RMS of ``a - b`` over the RMS of ``b``, both over the voxels ``inside``, in float64."""
    a, b = a[inside].astype(np.float64), b[inside].astype(np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def variation(x, inside):
    """Coefficient of variation (standard deviation over mean) of ``x`` over the voxels ``inside``, in float64."""
    v = x[inside].astype(np.float64)
    return float(v.std() / v.mean())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """Equal uint32 views wherever there is a number, NaNs in the same places (a NaN's sign and payload are nobody's rule)."""
    if not (a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))):
        return False
    number = ~np.isnan(a)
    return np.array_equal(bits(a)[number], bits(b)[number])
