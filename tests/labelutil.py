"""Masks and checks shared by tests/test_volume_label_host.py and tests/test_gpu_volume_label.py."""
import numpy as np


def bernoulli(shape, p, seed):
    return (np.random.default_rng(seed).uniform(size=shape) < p).astype(np.uint8)


def serpentine(shape=(64, 64, 80)):
    """A one-voxel-wide 6-connected path through the whole box: full z rows on even y, joined at alternating ends by one voxel
    on odd y; such sheets on even x, joined at alternating (y, z) corners by one voxel on odd x."""
    X, Y, Z = shape
    m = np.zeros(shape, dtype=np.uint8)
    for x in range(0, X, 2):
        end = 0                                                 # the z end at which the path stands
        for y in range(0, Y, 2):
            m[x, y, :] = 1
            end = Z - 1 - end
            if y + 2 < Y:
                m[x, y + 1, end] = 1
        if x + 2 < X:                                           # even sheets are left where they end, odd ones where they begin
            if (x // 2) % 2 == 0:
                m[x + 1, y, end] = 1
            else:
                m[x + 1, 0, 0] = 1
    return m


def check_canonical(lab, fg, offsets):
    """The label rule stated directly: 0 off the mask; equal across every neighbour pair; every label is 1 + the index of a voxel
    that carries it and no smaller index does."""
    flat = lab.reshape(-1)
    assert lab.dtype == np.int32 and np.array_equal(lab != 0, fg)
    for d in offsets:
        a = tuple(slice(max(0, -c), s - max(0, c)) for c, s in zip(d, fg.shape))
        b = tuple(slice(max(0, c), s - max(0, -c)) for c, s in zip(d, fg.shape))
        both = fg[a] & fg[b]
        assert np.array_equal(lab[a][both], lab[b][both])
    idx = np.flatnonzero(flat)
    assert (flat[idx] <= idx + 1).all()                         # no voxel before the one the label names
    assert (flat[flat[idx] - 1] == flat[idx]).all()             # the named voxel carries the label itself


def fixed_volume():
    rng = np.random.default_rng(42)
    v = np.abs(rng.normal(0, 30, (20, 24, 28)))
    x, y, z = np.meshgrid(*(np.linspace(-1, 1, s) for s in v.shape), indexing="ij")
    v[x * x + y * y + z * z < 0.4] += 900.0
    v[(x * x + y * y + z * z < 0.02)] = 5.0                     # a dark cavity
    v[1, 2, 3] = v[18, 20, 5] = 1200.0                          # two specks
    return np.rint(v).astype(np.float32)


def speck_volume(kind, shape=(33, 30, 45), seed=0):
    """A bright ball in a dark background, intensities in the style of the Otsu tests ("signed": two normal modes around -200
    and 150; "int12": integers, the bright ones multiples of 16 on bin edges), with a dark cavity at the centre of the ball, a dark
    notch of 3 x 3 voxels from inside the ball out along z (a hole only in the planes across z) and a few bright specks outside."""
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*(np.linspace(-1, 1, s) for s in shape), indexing="ij")
    r2 = x * x + y * y + z * z
    ball, cavity = r2 < 0.55, r2 < 0.04
    n = int(ball.sum())
    if kind == "signed":
        v = rng.normal(-200.0, 20.0, shape)
        v[ball] = rng.normal(150.0, 30.0, n)
        dark, bright = -200.0, 150.0
    else:
        v = np.rint(np.abs(rng.normal(0, 50, shape)))
        v[ball] = np.rint(rng.uniform(1600, 4096, n) / 16) * 16
        dark, bright = 0.0, 4096.0
    v[cavity] = dark
    v[15:18, 14:17, 33:] = dark
    for p in ((1, 2, 3), (31, 28, 40), (2, 27, 44), (30, 1, 0)):
        v[p] = bright
    v[1, 2, 4] = bright                                         # a speck of two voxels
    return v.astype(np.float32)
