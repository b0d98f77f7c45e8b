"""The numpy specification of the volume tools, pinned (no GPU): sha256 digests of what the public specification functions of
volume_reslice.py, volume_deform.py, volume_stacks.py and volume_slices.py return on small seeded inputs.

The digests below were computed with the code of commit 17180d0 ("Zero-filled x2 baseline and k-space truncation for volumes, in
HIP"), before the sampler, the Thirion rule and the registration frame of the specification were each brought down to one copy -
never with the code under test.  The specification is exact (every rounding fixed), so a change of a single bit anywhere in an
output changes its digest: this file says that the merged code is the same function as the copies it replaced.  An array enters a
digest with its dtype, its shape and its bytes, a float as ``float.hex()``, an integer as its decimal digits.
"""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import stackutil as U                                                        # noqa: E402
from mri_superresolution_amd import volume_deform as D                       # noqa: E402
from mri_superresolution_amd import volume_reslice as R                      # noqa: E402
from mri_superresolution_amd import volume_slices as SL                      # noqa: E402
from mri_superresolution_amd import volume_stacks as S                       # noqa: E402


def digest(*items) -> str:
    h = hashlib.sha256()

    def feed(x):
        if isinstance(x, (tuple, list)):
            h.update(b"(")
            for y in x:
                feed(y)
            h.update(b")")
        elif isinstance(x, np.ndarray):
            h.update(f"{x.dtype}{x.shape}".encode())
            h.update(np.ascontiguousarray(x).tobytes())
        elif isinstance(x, (float, np.floating)):
            h.update(float(x).hex().encode())
        elif isinstance(x, (int, np.integer)) and not isinstance(x, bool):
            h.update(str(int(x)).encode())
        else:
            raise TypeError(f"nothing of type {type(x)} goes into a digest")
        h.update(b";")

    feed(items)
    return h.hexdigest()


def matrix(angles, centre_dst, centre_src, shift=(0.0, 0.0, 0.0), scale=1.0):
    """Destination index -> source index: a rotation about the two centres, a scale and a shift."""
    m = np.zeros((3, 4))
    m[:, :3] = U.rotation(*angles) * scale
    m[:, 3] = np.asarray(centre_src) + np.asarray(shift) - m[:, :3] @ np.asarray(centre_dst)
    return m


# ---------------------------------------------------------------- reslice_np

RESLICE_SRC, RESLICE_DST = (5, 6, 7), (6, 5, 8)
RESLICE_M = matrix((10.0, 20.0, 30.0), (2.5, 2.0, 3.5), (2.0, 2.5, 3.0), shift=(0.3, -0.4, 0.2))


def test_the_reslice_case_has_voxels_inside_and_outside():
    share = 1.0 - R.source_coordinates_np(RESLICE_M, RESLICE_DST, RESLICE_SRC)[1].mean()
    assert 0.0 < share < 1.0


def reslice_case(method):
    v = np.random.default_rng(11).uniform(0.0, 900.0, RESLICE_SRC).astype(np.float32)
    return R.reslice_np(v, RESLICE_M, RESLICE_DST, method, fill=-3.0),


# ---------------------------------------------------------------- warp_np, warp_matrix_np, compose_np

FIELD_SHAPE = (6, 7, 8)


def rough_field(seed, sigma=2.0):
    """Displacements of a few voxels - many leave the volume - with one NaN, one +inf and one component far past a face."""
    u = np.random.default_rng(seed).normal(0.0, sigma, (3,) + FIELD_SHAPE).astype(np.float32)
    u[0, 1, 2, 3] = np.nan
    u[1, 2, 3, 4] = np.inf
    u[2, 0, 0, 7] = 5.0
    return u


def warp_case(method):
    moving = np.random.default_rng(12).uniform(0.0, 900.0, FIELD_SHAPE).astype(np.float32)
    return D.warp_np(moving, rough_field(13), method, fill=-3.0),


def warp_matrix_case(method):
    moving = np.random.default_rng(14).uniform(0.0, 900.0, (5, 6, 7)).astype(np.float32)
    m = matrix((-8.0, 12.0, 25.0), (2.5, 3.0, 3.5), (2.0, 2.5, 3.0), shift=(0.2, 0.1, -0.3), scale=0.9)
    return D.warp_matrix_np(moving, m, rough_field(15, sigma=1.0), method, fill=-3.0),


def compose_case():
    u = np.random.default_rng(16).normal(0.0, 1.5, (3,) + FIELD_SHAPE).astype(np.float32)
    v = rough_field(17, sigma=1.0)
    return D.compose_np(u, v), D.compose_np(v, v)


def test_the_field_cases_leave_the_volume_and_hold_the_special_values():
    u = rough_field(13)
    out = D.warp_np(np.ones(FIELD_SHAPE, dtype=np.float32), u, "linear", fill=-3.0)
    assert 0.0 < (out == -3.0).mean() < 1.0 and out[1, 2, 3] == -3.0 and out[2, 3, 4] == -3.0
    w = D.compose_np(rough_field(17, 1.0), rough_field(17, 1.0))
    assert np.isnan(w[:, 1, 2, 3]).all() and np.isinf(w[1, 2, 3, 4]) and np.isfinite(w[:, 0, 0, 7]).all()


# ---------------------------------------------------------------- the forces

@functools.lru_cache(maxsize=None)
def force_pair():
    """(8, 9, 10): a corner where both scans are one constant and the field is zero (no gradient, no difference: den <= DEN_MIN)
    and a voxel that is not finite in each scan."""
    rng = np.random.default_rng(18)
    fixed = rng.uniform(0.0, 900.0, (8, 9, 10)).astype(np.float32)
    moving = (0.6 * fixed + rng.uniform(0.0, 300.0, fixed.shape)).astype(np.float32)
    u = rng.normal(0.0, 0.7, (3,) + fixed.shape).astype(np.float32)
    fixed[:4, :4, :4] = moving[:4, :4, :4] = 100.0
    u[:, :4, :4, :4] = 0.0
    moving[5, 5, 5] = np.nan
    fixed[6, 2, 7] = np.inf
    return fixed, moving, u


def test_the_force_case_reaches_the_denominator_guard():
    fixed, moving, u = force_pair()
    w, _ = D.demons_update_np(fixed, moving, u, 0.1)
    g = D.gradient_np(fixed)
    assert (g[:, :3, :3, :3] == 0).all() and (moving[:3, :3, :3] == fixed[:3, :3, :3]).all() and not u[:, :3, :3, :3].any()
    assert not w[:, :3, :3, :3].any() and np.abs(w).max() == np.float32(0.1)      # the guard and the clamp are both reached


def force_case(name):
    fixed, moving, u = force_pair()
    if name == "demons_force":
        return D.demons_force_np(fixed, moving, u, 0.1, fill=50.0)
    if name == "demons_update":
        return D.demons_update_np(fixed, moving, u, 0.1, fill=50.0, scale=0.25)
    kind, radius = name.rsplit("_r", 1)
    if kind == "lcc_force":
        return D.lcc_force_np(fixed, moving, u, int(radius), 0.1)
    return D.lcc_update_np(fixed, moving, u, int(radius), 0.1, scale=0.25)


# ---------------------------------------------------------------- the registrations

@functools.lru_cache(maxsize=None)
def register_pair():
    x = np.meshgrid(*(np.arange(16, dtype=np.float64),) * 3, indexing="ij")
    r = np.sqrt(sum((x[a] - c) ** 2 for a, c in enumerate((7.5, 7.0, 8.0))))
    fixed = (600.0 / (1.0 + np.exp(r - 5.0)) + 20.0 * np.sin(x[0] + 0.5 * x[1]) * np.cos(0.7 * x[2])).astype(np.float32)
    r = np.sqrt(sum((x[a] - c) ** 2 for a, c in enumerate((8.3, 7.4, 7.2))))
    moving = (600.0 / (1.0 + np.exp(r - 5.5)) + 20.0 * np.sin(x[0] + 0.5 * x[1]) * np.cos(0.7 * x[2])).astype(np.float32)
    return fixed, moving


def register_case(kind, force, exp_steps=None):
    fixed, moving = register_pair()
    kw = dict(levels=2, iterations=(2, 1), force=force, lcc_radius=1)
    got = D.register_deformable_np(fixed, moving, **kw) if kind == "deformable" else \
        D.register_diffeomorphic_np(fixed, moving, exp_steps=exp_steps, **kw)
    assert got.schedule == (((8, 8, 8), 2), ((16, 16, 16), 1)) and len(got.stats) == 3
    return got.field, got.warped, [tuple(row) for row in got.stats], tuple(got.jacobian)


# ---------------------------------------------------------------- the stacks

@functools.lru_cache(maxsize=None)
def stack_set():
    """Three orthogonal stacks, 3 voxels thick, of a (12, 15, 17) volume: the smallest set of tests/test_volume_stacks_host.py."""
    truth = np.random.default_rng(19).uniform(0.0, 900.0, (12, 15, 17)).astype(np.float32)
    return (truth,) + tuple(U.orthogonal_stacks(truth, 3)[:2])


def stacks_case(name):
    truth, stacks, geometries = stack_set()
    x = np.random.default_rng(20).uniform(0.0, 900.0, truth.shape).astype(np.float32)
    if name == "simulate":
        a = U.oblique_affine(truth.shape, (8, 9, 4), (1.5, 1.5, 4.0))
        g = S.stack_geometry(a, np.eye(4), 2, samples=3)
        return S.simulate_stack_np(truth, g, (8, 9, 4), fill=-1.0), [s.copy() for s in stacks]
    if name == "residual":
        return [S.stack_residual_np(x, y, g) for y, g in zip(stacks, geometries)]
    if name == "update":
        return S.stack_update_np(x, stacks, geometries, 0.7, clamp=100.0)
    if name == "combine":
        got = S.combine_stacks_np(stacks, geometries, truth.shape, iterations=2, step=0.8)
        return got.volume, got.initial, np.asarray(got.rms, dtype=np.float64), np.asarray(got.counts, dtype=np.int64)
    g, y = geometries[2], stacks[2]                                          # "slices": a pose per slice
    table = np.stack([np.asarray(g.to_output, dtype=np.float64) + 0.01 * s * np.eye(3, 4, k=s % 3) for s in range(y.shape[2])])
    return SL.simulate_stack_slices_np(x, g, y.shape, table, fill=-1.0), SL.stack_residual_slices_np(x, y, g, table)


# ---------------------------------------------------------------- the digests

CASES = {
    "reslice_nearest": (reslice_case, "nearest"), "reslice_linear": (reslice_case, "linear"), "reslice_cubic": (reslice_case, "cubic"),
    "warp_linear": (warp_case, "linear"), "warp_cubic": (warp_case, "cubic"),
    "warp_matrix_linear": (warp_matrix_case, "linear"), "warp_matrix_cubic": (warp_matrix_case, "cubic"),
    "compose": (compose_case,),
    "demons_force": (force_case, "demons_force"), "demons_update": (force_case, "demons_update"),
    "lcc_force_r1": (force_case, "lcc_force_r1"), "lcc_force_r2": (force_case, "lcc_force_r2"),
    "lcc_update_r1": (force_case, "lcc_update_r1"), "lcc_update_r2": (force_case, "lcc_update_r2"),
    "deformable_ssd": (register_case, "deformable", "ssd"), "deformable_lcc": (register_case, "deformable", "lcc"),
    "diffeomorphic_ssd_exp0": (register_case, "diffeomorphic", "ssd", 0), "diffeomorphic_ssd_exp2": (register_case, "diffeomorphic", "ssd", 2),
    "diffeomorphic_lcc_exp0": (register_case, "diffeomorphic", "lcc", 0), "diffeomorphic_lcc_exp2": (register_case, "diffeomorphic", "lcc", 2),
    "stacks_simulate": (stacks_case, "simulate"), "stacks_residual": (stacks_case, "residual"), "stacks_update": (stacks_case, "update"),
    "stacks_combine": (stacks_case, "combine"), "stacks_slices": (stacks_case, "slices"),
}

PINNED = {
    "reslice_nearest": "1174eab4f8b100e0bf2bf19cb1014063847b42e2f3e0b16a28159d3789332d21",
    "reslice_linear": "12d4f84dd76e5c61b261bcee79764257ec9e1292816d0e3754f3447385fe02cb",
    "reslice_cubic": "c1c57dc3becaad921b47422f4de618ab8231d4f22ecdb1bf67367f121fb06598",
    "warp_linear": "30173ab54aa12f7fe534b8e1e79198cbe2345aaad77ffd9e3dcb11ffd0f786fd",
    "warp_cubic": "2cdeb55272ca05886d0a8a4f5fc7265ee60ea1223f3a245362c8e0ec451ca59f",
    "warp_matrix_linear": "c4210ffb7f2288d0d857fd0ac97ebd8ac35ae2cf47fb3ae0450252b564ca66ea",
    "warp_matrix_cubic": "dfdc16ad36ab113eecd8eefaf22fa9469d181d54e9f3bbe5f5fd99209be3aee0",
    "compose": "a1887522017d04015eec5cfd778cbaf06e9c73b8ced5d3b6f64b593bb12da6e7",
    "demons_force": "7d2e0636833a6d6e619aa6568dfad14138b750813474f0b8b41f6b74c0338b01",
    "demons_update": "41f58d37f1e6e88312ee5ea5df1fda32dc4994850f5e22a9dd1826f6dcbf10db",
    "lcc_force_r1": "cf6a628ee4fc08526b6f3f230cd055b79298a43e227ea3f1f3866f10e0e7b3b6",
    "lcc_force_r2": "8c123bcd32124dd45c26f87491d6e532fdde28b22b8c45c21338cf8f9ce2039f",
    "lcc_update_r1": "ed297ce9d781588675b872c7f5610040eeddc12cda0392e7a018817ee8679aeb",
    "lcc_update_r2": "ab1641bce8d164b81f5c3a576facb16549ff18d009a1e7aba299c963b4c119f9",
    "deformable_ssd": "726915335765d53b9ce18d7e2bd904cc1c5a4c945bb566bd8f1a9d5eafee75aa",
    "deformable_lcc": "93e56bf625496e410c18f8fc05c509a543c67e20ea7ab59303b37ffbbbc9e1f7",
    "diffeomorphic_ssd_exp0": "cd36fb74c7cea5c0f069ba877f146698ed558f41a81ff7bb5d0edc5a09df3236",
    "diffeomorphic_ssd_exp2": "cfa4ec4c380ee28f683bc3ad47ff17d2f76480ebfac4411445ad4ec1d5142d3a",
    "diffeomorphic_lcc_exp0": "57913b7fc4387390a2740a4650596663e424f651845d908f4b4869bcde0347d3",
    "diffeomorphic_lcc_exp2": "745aff9b261477b2c32df0c279765d168c932e47205bea54014735b79519799e",
    "stacks_simulate": "b39053e8849edbb4fe5f36b30a823644cc58be2c5b57762232018419a7b9e770",
    "stacks_residual": "c2eb1fe45ea30e14f22a3b68a6b72cf630ae08bec8b2746e8790039bb31bae39",
    "stacks_update": "29890b8af5a09f34b43e8e9b7589facabe11f96b7cb8b76488ee89465275387b",
    "stacks_combine": "1f17e547c62238c69b0b641e086f2c4c63f365ade76ac985a08643b6e70ed54d",
    "stacks_slices": "eec2fbe607fd10296e10e17cb88c5c8b3d70bbc3540e6a1d5a9522c8bb504641",
}


def test_every_case_is_pinned():
    assert sorted(PINNED) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_specification_returns_the_pinned_bits(name):
    fn, *args = CASES[name]
    assert digest(*fn(*args)) == PINNED[name]
