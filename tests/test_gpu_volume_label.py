"""Connected-component clean-up of foreground masks (GPU): csrc/volume_label.hip against label_components_np,
largest_component_np and fill_holes_np, foreground_mask(largest=, fill_holes=) against foreground_mask_np,
evaluate_volume(mask_largest=, mask_fill_holes=) and scripts/evaluate_volume.py --mask_largest --mask_fill_holes --save_mask.

Everything here is bit-equal to the numpy specification (labels are 1 + the smallest C-order index of the component, so the order
of the atomics cannot show), except the metric rows, which are compared with volume_metrics(mask=<the specification's mask>) at
rtol 1e-12: the same kernel on the same mask, only the order of its double sums is free (tests/test_gpu_volume_mask.py)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mri_superresolution_amd import _lib as L                                # noqa: E402
from mri_superresolution_amd import volume_eval as V                         # noqa: E402
from mri_superresolution_amd.models.unet_model import UNetSuperRes          # noqa: E402
from mri_superresolution_amd.utils.nifti import NiftiHeader, read_nifti, write_nifti      # noqa: E402
from scripts import evaluate_volume as cli                                   # noqa: E402
from labelutil import bernoulli, serpentine, speck_volume                   # noqa: E402

# one tile of 8 x 8 x 32; ragged tiles on every axis; many tiles
SHAPES = [(1, 1, 1), (3, 5, 7), (17, 9, 33), (70, 37, 45), (64, 64, 80)]
DENSITIES = [0.1, 0.3, 0.5, 0.9]      # both percolation thresholds lie inside: thousands of small components ... one that spans


@functools.lru_cache(maxsize=None)
def spec_labels(shape, p, conn, axis=None, invert=False):
    return V.label_components_np(mask_of(shape, p), conn, axis, invert)


@functools.lru_cache(maxsize=None)
def mask_of(shape, p):
    if p == 0.0 or p == 1.0:
        return np.full(shape, int(p) * 3, dtype=np.uint8)          # any non-zero value is foreground
    m = bernoulli(shape, p, seed=sum(shape) + int(10 * p))
    m.setflags(write=False)
    return m


def gpu_labels(m, conn, axis=None, invert=False):
    lab = V.label_components(torch.from_numpy(np.ascontiguousarray(m)).cuda(), conn, axis, invert)
    assert lab.dtype == torch.int32 and lab.is_cuda and tuple(lab.shape) == m.shape
    return lab.cpu().numpy()


def same(got, want, what):
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} differ, first at {np.argwhere(bad)[0]}"


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_labels_are_bit_equal_to_the_specification(shape, connectivity):
    for p in [0.0] + DENSITIES + [1.0]:
        want = spec_labels(shape, p, connectivity)
        same(gpu_labels(mask_of(shape, p), connectivity), want, f"{shape} p {p} c{connectivity}")
    print(f"{shape} c{connectivity}: components at p = {DENSITIES}: "
          f"{[len(np.unique(spec_labels(shape, p, connectivity))) - 1 for p in DENSITIES]}")
    full = spec_labels(shape, 1.0, connectivity)
    assert (full == 1).all() and not spec_labels(shape, 0.0, connectivity).any()


@pytest.mark.parametrize("shape", [(17, 9, 33), (70, 37, 45)], ids=str)
def test_plane_mode_and_invert(shape):
    m = mask_of(shape, 0.5)
    for conn in (6, 26):
        for axis in (0, 1, 2):
            same(gpu_labels(m, conn, axis), spec_labels(shape, 0.5, conn, axis), f"{shape} c{conn} plane {axis}")
        for axis in (None, 1):
            got = gpu_labels(m, conn, axis, invert=True)
            same(got, spec_labels(shape, 0.5, conn, axis, True), f"{shape} c{conn} plane {axis} inverted")
            same(got, gpu_labels(1 - m, conn, axis), "invert against the complement")
    bool_mask = torch.from_numpy(m != 0).cuda()                  # a bool mask is the same mask
    same(V.label_components(bool_mask, 26).cpu().numpy(), spec_labels(shape, 0.5, 26), "bool mask")
    with pytest.raises(ValueError):
        V.label_components(bool_mask.float())
    with pytest.raises(ValueError, match="connectivity"):
        V.label_components(bool_mask, 18)


def test_checkerboard_and_serpentine():
    x, y, z = np.meshgrid(*(np.arange(s) for s in (17, 9, 33)), indexing="ij")
    board = ((x + y + z) % 2 == 0).astype(np.uint8)
    got26, got6 = gpu_labels(board, 26), gpu_labels(board, 6)
    assert np.array_equal(np.unique(got26), [0, 1])              # one component through the corners
    same(got6.reshape(-1), np.where(board.reshape(-1) != 0, np.arange(1, board.size + 1), 0), "singletons")
    # the deepest merge chain: one path through every tile of the box, thousands of tile crossings
    m = serpentine((64, 64, 80))
    want = V.label_components_np(m, 6)
    assert np.array_equal(np.unique(want), [0, 1])               # by the specification: one component
    same(gpu_labels(m, 6), want, "serpentine c6")
    same(gpu_labels(m, 26), V.label_components_np(m, 26), "serpentine c26")
    kept, st = V.largest_component(torch.from_numpy(m).cuda(), 6)
    same(kept.cpu().numpy(), m, "serpentine kept")
    assert st.cpu().tolist() == [1.0, float(m.sum()), 1.0]


def guarded(fn, n, dtype, margin):
    """fn(pointer) writes n items of dtype into the middle of a buffer of 7s -> the items, after checking the guard cells."""
    buf = torch.full((n + 2 * margin,), 7, dtype=dtype, device="cuda")
    assert fn(buf.data_ptr() + margin * buf.element_size()) == 0
    b = buf.cpu().numpy()
    assert (b[:margin] == 7).all() and (b[margin + n:] == 7).all()
    return b[margin:margin + n]


def test_entry_points_inside_guard_cells_and_off_alignment():
    """labels, dst inside larger buffers of 7s; dst on and 1 byte off a 4-byte boundary (word and byte stores), the mask off it too."""
    lib, st = L.load(), L.stream_ptr()
    shape = (70, 37, 45)
    m = mask_of(shape, 0.3)
    n = m.size
    src = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    ws = torch.empty(int(lib.mrisr_u8_volume_label_workspace_bytes(*shape)) // 8, dtype=torch.int64, device="cuda")
    assert ws.numel() * 8 == 64 + 8 * n
    stats = torch.full((4,), -1.0, dtype=torch.float64, device="cuda")
    want_kept, want_st = V.largest_component_np(m, 26)
    want_fill, want_filled = V.fill_holes_np(mask_of(shape, 0.8))
    for off, margin in ((0, 64), (3, 61)):
        mp = src.data_ptr() + off
        src[off:off + n] = torch.from_numpy(m).cuda().reshape(-1)
        lab = guarded(lambda p: lib.mrisr_u8_volume_label(mp, *shape, 26, -1, 0, p, st), n, torch.int32, 64)
        same(lab.reshape(shape), spec_labels(shape, 0.3, 26), "labels in guard cells")
        kept = guarded(lambda p: lib.mrisr_u8_volume_keep_largest(mp, *shape, 26, p, stats.data_ptr(), ws.data_ptr(), st), n, torch.uint8, margin)
        same(kept.reshape(shape), want_kept, f"kept, margin {margin}")
        assert stats.cpu().tolist() == want_st.tolist() + [-1.0]
        src[off:off + n] = torch.from_numpy(mask_of(shape, 0.8)).cuda().reshape(-1)
        filled = guarded(lambda p: lib.mrisr_u8_volume_fill_holes(mp, *shape, -1, p, stats.data_ptr() + 24, ws.data_ptr(), st), n, torch.uint8,
                         margin)
        same(filled.reshape(shape), want_fill, f"filled, margin {margin}")
        assert stats.cpu().tolist() == want_st.tolist() + [float(want_filled)]
        stats[3] = -1.0
        assert np.array_equal(src[off:off + n].cpu().numpy().reshape(shape), mask_of(shape, 0.8))      # the source is left alone
    # refusals launch nothing
    assert lib.mrisr_u8_volume_keep_largest(src.data_ptr(), *shape, 26, src.data_ptr(), stats.data_ptr(), ws.data_ptr(), st) == -1
    assert lib.mrisr_u8_volume_fill_holes(src.data_ptr(), *shape, 3, src.data_ptr() + 4, stats.data_ptr(), ws.data_ptr(), st) == -1
    assert lib.mrisr_u8_volume_label(src.data_ptr(), 70, 0, 45, 26, -1, 0, ws.data_ptr(), st) == -2
    dst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    for bad in ((0, 37, 45), (70, 32768, 45), (70, 37, -1)):
        assert lib.mrisr_u8_volume_keep_largest(src.data_ptr(), *bad, 26, dst.data_ptr(), stats.data_ptr(), ws.data_ptr(), st) == -2
        assert lib.mrisr_u8_volume_fill_holes(src.data_ptr(), *bad, -1, dst.data_ptr(), stats.data_ptr(), ws.data_ptr(), st) == -2
        assert lib.mrisr_u8_volume_label_workspace_bytes(*bad) == 0


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_largest_component_and_its_statistics(shape):
    for p in (0.0, 0.1, 0.3, 0.9, 1.0):
        m = mask_of(shape, p)
        for conn in (6, 26):
            kept, st = V.largest_component(torch.from_numpy(m).cuda(), conn)
            want, want_st = V.largest_component_np(m, conn)
            assert kept.dtype == torch.uint8 and st.dtype == torch.float64 and st.is_cuda
            same(kept.cpu().numpy(), want, f"{shape} p {p} c{conn}")
            assert st.cpu().tolist() == want_st.tolist(), (shape, p, conn)
    if min(shape) < 9:
        return
    # two boxes of one size: the one with the smaller label is kept; one more voxel turns it round
    m = np.zeros(shape, dtype=np.uint8)
    m[1:3, 1:4, 1:5] = 1
    m[shape[0] - 4:shape[0] - 2, 4:7, shape[2] - 6:shape[2] - 2] = 1
    m[0, 8, 0] = 1
    kept, st = V.largest_component(torch.from_numpy(m).cuda())
    assert st.cpu().tolist() == [3.0, 24.0, float(np.ravel_multi_index((1, 1, 1), shape) + 1)]
    assert kept.cpu().numpy()[1:3, 1:4, 1:5].all() and int(kept.sum()) == 24
    m[shape[0] - 4, 4, shape[2] - 7] = 1
    kept, st = V.largest_component(torch.from_numpy(m).cuda())
    assert st.cpu().tolist()[:2] == [3.0, 25.0] and kept.cpu().numpy()[1:3, 1:4, 1:5].sum() == 0 and int(kept.sum()) == 25


def test_fill_holes_shell_pin_hole_diagonal_gap_and_random_masks():
    shape = (17, 19, 40)                                         # the shell spans tiles on every axis
    shell = np.zeros(shape, dtype=np.uint8)
    shell[2:15, 2:17, 2:38] = 1
    shell[3:14, 3:16, 3:37] = 0
    cavity = 11 * 13 * 34
    pin, gap = shell.copy(), shell.copy()
    pin[2, 9, 20] = 0                                            # a one-voxel channel through a face
    gap[2, 2, 2] = 0                                             # the shell's corner: only diagonal to the cavity
    for name, m, count in (("shell", shell, cavity), ("pin-hole", pin, 0), ("diagonal gap", gap, cavity)):
        got, filled = V.fill_holes(torch.from_numpy(m).cuda())
        want, want_count = V.fill_holes_np(m)
        assert want_count == count, name                         # the specification does what the case is named for
        same(got.cpu().numpy(), want, name)
        assert filled.dtype == torch.float64 and filled.is_cuda and filled.dim() == 0 and float(filled) == count
        for axis in (0, 1, 2):
            got, filled = V.fill_holes(torch.from_numpy(m).cuda(), axis)
            want, want_count = V.fill_holes_np(m, axis)
            same(got.cpu().numpy(), want, f"{name} plane {axis}")
            assert float(filled) == want_count
    for p in (0.6, 0.8):
        m = mask_of((70, 37, 45), p)
        for axis in (None, 0, 1, 2):
            got, filled = V.fill_holes(torch.from_numpy(m).cuda(), axis)
            want, want_count = V.fill_holes_np(m, axis)
            print(f"p {p} axis {axis}: {want_count} voxels filled")
            assert want_count > 1000
            same(got.cpu().numpy(), want, f"p {p} axis {axis}")
            assert float(filled) == want_count
    for shape in SHAPES[:3]:
        for p in (0.0, 0.5, 1.0):
            m = mask_of(shape, p)
            got, filled = V.fill_holes(torch.from_numpy(m).cuda())
            want, want_count = V.fill_holes_np(m)
            same(got.cpu().numpy(), want, f"{shape} p {p}")
            assert float(filled) == want_count and got.max() <= 1
    with pytest.raises(ValueError, match="axis"):
        V.fill_holes(torch.from_numpy(shell).cuda(), 3)


@pytest.mark.parametrize("kind", ["signed", "int12"])
def test_foreground_mask_with_clean_up_against_the_specification(kind):
    v = speck_volume(kind, seed=3)
    x = torch.from_numpy(v).cuda()
    plain, stats0 = V.foreground_mask(x, 1)
    assert stats0.cleanup is None and np.array_equal(plain.cpu().numpy(), V.foreground_mask_np(v, 1))
    seen = set()
    for largest, fill in ((True, None), (False, "3d"), (True, "3d"), (True, 0), (True, 1), (False, 2)):
        mask, stats = V.foreground_mask(x, 1, largest=largest, fill_holes=fill)
        want, st = V.foreground_mask_np(v, 1, return_stats=True, largest=largest, fill_holes=fill)
        same(mask.cpu().numpy(), want, f"{kind} largest {largest} fill {fill}")
        assert stats.cpu().tolist() == stats0.cpu().tolist() == [float(st["lo"]), float(st["hi"]), float(st["t"]), float(st["count"])]
        got = stats.cleanup.cpu().numpy()
        assert got.dtype == np.float64 and np.array_equal(got, st["cleanup"], equal_nan=True), (got, st["cleanup"])
        print(f"{kind} largest {largest} fill {fill}: cleanup {got}, {int(want.sum())} voxels")
        if largest:
            assert got[0] == 5 and want[1, 2, 3] == 0 and want[31, 28, 40] == 0      # the ball and four specks
        if fill is not None:
            assert got[2] > 0 and want[16, 15, 22] == 1          # the cavity at the centre
            assert want[16, 15, 34] == (1 if fill == 2 else 0)   # the notch: a hole only in the planes across z
        seen.add(want.tobytes())
    assert len(seen) >= 4                                        # the options do different things on this volume


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(1234)
    return UNetSuperRes(1, 1, base_filters=16).cuda().eval()     # 16: the narrowest the engine builds


def small_reference():
    """16 x 16 x 16: a bright block with a dark cavity, specks in two corners."""
    rng = np.random.default_rng(9)
    v = np.abs(rng.normal(0, 20, (16, 16, 16)))
    v[3:13, 3:13, 3:13] = 1000 + rng.normal(0, 30, (10, 10, 10))
    v[6:9, 6:9, 6:9] = 10.0
    v[0, 0, 1] = v[15, 14, 15] = 1100.0
    return np.rint(v).astype(np.float32)


def test_evaluate_volume_with_clean_up(model):
    full = small_reference()
    ref = torch.from_numpy(full).cuda()
    kw = dict(batch_size=4, use_graph=False)
    plain = V.evaluate_volume(model, ref, **kw)
    masked = V.evaluate_volume(model, ref, mask="otsu", **kw)
    assert masked.mask_cleanup is None
    res = V.evaluate_volume(model, ref, mask="otsu", mask_largest=True, mask_fill_holes="3d", **kw)
    want_mask, st = V.foreground_mask_np(full, 0, return_stats=True, largest=True, fill_holes="3d")
    same(res.mask.cpu().numpy(), want_mask, "the mask scored")
    assert want_mask.sum() == 1000 and st["cleanup"].tolist() == [3.0, 973.0, 27.0]
    assert res.mask_cleanup.dtype == torch.float64 and res.mask_cleanup.is_cuda and res.mask_cleanup.cpu().tolist() == [3.0, 973.0, 27.0]
    assert float(res.mask_count) == 1000.0 and float(masked.mask_count) == 975.0
    assert res.mask_stats.cpu().tolist() == masked.mask_stats.cpu().tolist()
    rng = float(full.max() - full.min())
    lr = V.downsample2(ref, (0, 1))
    spec_mask = torch.from_numpy(want_mask).cuda()
    for method in ("linear", "cubic"):
        direct = V.volume_metrics(V.upscale2(lr, method, (0, 1)), ref, rng, mask=spec_mask)
        assert torch.allclose(res[method], direct, rtol=1e-12, atol=0), method
    for k in plain:
        assert torch.allclose(res[k][0], plain[k], rtol=1e-12, atol=0) and torch.allclose(masked[k][0], plain[k], rtol=1e-12, atol=0)
        assert not torch.allclose(res[k][1], masked[k][1], rtol=1e-6, atol=0)      # 25 other voxels: another foreground row
    # a given mask is cleaned the same way; without the new flags it is what it was
    given = torch.from_numpy(V.foreground_mask_np(full)).cuda()
    same_given = V.evaluate_volume(model, ref, mask=given, mask_largest=True, mask_fill_holes="3d", **kw)
    assert same_given.mask_stats is None and same_given.mask_cleanup.cpu().tolist() == [3.0, 973.0, 27.0]
    untouched = V.evaluate_volume(model, ref, mask=given, **kw)
    assert untouched.mask_cleanup is None
    for k in plain:
        assert torch.allclose(same_given[k], res[k], rtol=1e-12, atol=0) and torch.allclose(untouched[k], masked[k], rtol=1e-12, atol=0)
    only_fill = V.evaluate_volume(model, ref, mask="otsu", mask_fill_holes=2, **kw)
    c = only_fill.mask_cleanup.cpu().numpy()
    assert np.isnan(c[:2]).all() and c[2] == 27.0 and float(only_fill.mask_count) == 1002.0
    with pytest.raises(ValueError, match="need a mask"):
        V.evaluate_volume(model, ref, mask_largest=True, **kw)


def test_command_line_with_clean_up_and_save_mask(model, tmp_path, capsys):
    ckdir = tmp_path / "ck"
    ckdir.mkdir()
    torch.save({"model_state_dict": {k: v.cpu() for k, v in model.state_dict().items()}}, ckdir / "best_model_unet.pth")
    vol = np.concatenate([small_reference(), np.zeros((1, 16, 16), dtype=np.float32)], axis=0)      # 17: the odd extent is cropped
    vol4 = np.stack([vol, vol[:, ::-1].copy()], axis=3)
    one, two = tmp_path / "scan.nii.gz", tmp_path / "scan4d.nii"
    write_nifti(str(one), vol, NiftiHeader.new(vol.shape, (1.0, 1.0, 1.0)), ())
    write_nifti(str(two), vol4, NiftiHeader.new(vol4.shape, (1.0, 1.0, 1.0, 2.0)), ())
    common = ["--checkpoint_dir", str(ckdir), "--base_filters", "16", "--batch_size", "4", "--no_graph"]
    out = tmp_path / "mask.nii.gz"
    capsys.readouterr()
    flags = ["--mask", "otsu", "--mask_largest", "--mask_fill_holes", "3d"]
    assert cli.main(cli.parse_args(["--reference", str(one), "--save_mask", str(out)] + flags + common)) == 0
    text = capsys.readouterr().out
    assert "foreground: 1000 voxels, 24.4 % of the volume, Otsu threshold " in text
    assert text.count(", 3 components, kept 973 voxels, filled 27\n") == 1
    res = V.evaluate_volume(model, torch.from_numpy(vol).cuda(), batch_size=4, use_graph=False, mask="otsu", mask_largest=True,
                            mask_fill_holes="3d")
    data, hdr = read_nifti(str(out))
    assert tuple(data.shape) == (16, 16, 16) and hdr.get("datatype") == 2 and hdr.get("bitpix") == 8
    same(data.astype(np.uint8), res.mask.cpu().numpy(), "--save_mask")
    # a 4-D reference gives a 4-D mask; only the planes' holes with an axis
    out4 = tmp_path / "mask4d.nii"
    assert cli.main(cli.parse_args(["--reference", str(two), "--save_mask", str(out4), "--mask", "otsu", "--mask_fill_holes", "2"] + common)) == 0
    text = capsys.readouterr().out
    assert text.count(", filled 27\n") == 2 and "components" not in text
    data4, _ = read_nifti(str(out4))
    assert tuple(data4.shape) == (16, 16, 16, 2)
    for t in range(2):
        want = V.foreground_mask_np(np.ascontiguousarray(vol4[:16, :, :, t]), fill_holes=2)
        same(data4[..., t].astype(np.uint8), want, f"timepoint {t}")
    # without the new flags: the title line of before
    assert cli.main(cli.parse_args(["--reference", str(one), "--mask", "otsu"] + common)) == 0
    text = capsys.readouterr().out
    assert "foreground: 975 voxels" in text and "components" not in text and "filled" not in text
    # the three options need --mask; --save_mask takes one reference
    assert cli.main(cli.parse_args(["--reference", str(one), "--mask_largest"] + common)) == 1
    assert cli.main(cli.parse_args(["--reference", str(one), "--mask_fill_holes", "3d"] + common)) == 1
    assert cli.main(cli.parse_args(["--reference", str(one), "--save_mask", str(out)] + common)) == 1
    assert cli.main(cli.parse_args(["--reference", str(one), str(two), "--mask", "otsu", "--save_mask", str(out)] + common)) == 1
