"""Isotropic x2 volumes (GPU): csrc/volume_blend.hip against volume.combine_planes_np bit for bit, enhance_volume_isotropic
against the combination of the three enhance_volume passes, and scripts/infer_volume.py --isotropic.

Bars.  The kernel restates combine_planes_np operation by operation, and the eager forward is deterministic: both comparisons
are bit-equal.  A graph replay and the eager forward agree per slice within the project's fp32 bar, 1e-3 of the slice's window
(tests/test_gpu_volume.py); the through-plane rule is a convex combination of a slice and one neighbour and the blend a mean of
the planes, so an output voxel is within 1e-3 of the mean over the planes of the widest window among the slices it draws on
(plus the float32 rounding of the combination itself, four ulp of the intensity scale)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mri_superresolution_amd import _lib as L                                # noqa: E402
from mri_superresolution_amd.models.unet_model import UNetSuperRes          # noqa: E402
from mri_superresolution_amd.utils import imageops                           # noqa: E402
from mri_superresolution_amd.utils.nifti import NiftiHeader, read_nifti, write_nifti   # noqa: E402
from mri_superresolution_amd.volume import combine_planes_np, enhance_volume, enhance_volume_isotropic, up2_blend   # noqa: E402
from scripts import infer_volume                                             # noqa: E402

BAR = 1e-3
E_ARG, E_SHAPE = -1, -2      # MRISR_E_ARG, MRISR_E_SHAPE (include/mrisr.h)
CONSTANT_SLICE, CONSTANT_VALUE = 1, 1234.0


# ---------------------------------------------------------------- the kernel alone

def random_planes(dims, seed, scale=3000.0, step=None):
    """{axis: E_axis} for an input volume of dims: axis kept, the two others doubled; values in +-scale (multiples of step)."""
    rng = np.random.default_rng(seed)
    planes = {}
    for a in range(3):
        shape = tuple(d if i == a else 2 * d for i, d in enumerate(dims))
        v = rng.uniform(-scale, scale, shape)
        planes[a] = (np.rint(v / step) * step if step else v).astype(np.float32)
    return planes


def off_boundary(shape, dtype, fill, off):
    """A contiguous tensor of this shape whose base lies off elements past a 16-byte boundary."""
    n = int(np.prod(shape))
    return torch.full((n + off,), fill, dtype=dtype, device="cuda")[off:].view(shape)


def slice_major(e, axis, off=0):
    e = np.ascontiguousarray(np.moveaxis(e, axis, 0))
    x = off_boundary(e.shape, torch.float32, 0.0, off)
    x.copy_(torch.from_numpy(e))
    return x


def run_blend(planes, dims, out_dtype, off=0):
    """SET -> ADD -> FINISH over the planes in ascending order; a float32 result is finished in place (out is acc).  ``off``: every
    float32 buffer starts that many floats, the int16 output twice as many values, past a 16-byte boundary."""
    full = tuple(2 * d for d in dims)
    axes = sorted(planes)
    acc = off_boundary(full, torch.float32, float("nan"), off)                         # SET must not read it
    out = acc if out_dtype == torch.float32 else off_boundary(full, torch.int16, -1, 2 * off)
    assert acc.data_ptr() % 16 == 4 * off and out.data_ptr() % 16 == 4 * off
    for i, a in enumerate(axes):
        last = i == len(axes) - 1
        up2_blend(slice_major(planes[a], a, off), a, acc, L.VOLBLEND_FINISH if last else (L.VOLBLEND_SET if i == 0 else L.VOLBLEND_ADD),
                  len(axes), out if last else None)
    return out.cpu().numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32 if a.dtype == np.float32 else np.int16),
                                                                        b.view(np.int32 if b.dtype == np.float32 else np.int16))


# S = 1 and S = 2 on every axis, rows that are no multiple of 4; (33, 17, 65) crosses a 32- and a 64-wide tile edge in every
# direction of the transposing form with halo at both ends; (64, 32, 16) is the aligned, whole-tile case
KERNEL_DIMS = [(1, 3, 5), (2, 1, 7), (5, 7, 1), (3, 4, 2), (33, 17, 65), (64, 32, 16)]


@pytest.mark.parametrize("dims", KERNEL_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_blend_sequence_is_bit_equal_to_the_numpy_specification(dims):
    planes = random_planes(dims, seed=sum(dims))
    for np_dtype, dtype in ((np.float32, torch.float32), (np.int16, torch.int16)):
        got, want = run_blend(planes, dims, dtype), combine_planes_np(planes, np_dtype)
        assert same_bits(got, want), (dims, dtype, int((got != want).sum()))
    for axis in (0, 1, 2):                                      # FINISH as the first and only plane: out = U(plane)
        for np_dtype, dtype in ((np.float32, torch.float32), (np.int16, torch.int16)):
            got, want = run_blend({axis: planes[axis]}, dims, dtype), combine_planes_np({axis: planes[axis]}, np_dtype)
            assert same_bits(got, want), (dims, axis, dtype)
    two = {0: planes[0], 2: planes[2]}                          # a mean of two: SET -> FINISH with count 2
    assert same_bits(run_blend(two, dims, torch.float32), combine_planes_np(two))


def test_blend_sequence_off_a_16_byte_boundary():
    """5 x 7 x 9 input voxels (no multiple of 4); planes, accumulator and output 8 bytes past a 16-byte boundary: the stream
    form takes its 8-byte path, the transposing form pairs."""
    dims = (5, 7, 9)
    planes = random_planes(dims, seed=sum(dims))
    for np_dtype, dtype in ((np.float32, torch.float32), (np.int16, torch.int16)):
        got, want = run_blend(planes, dims, dtype, off=2), combine_planes_np(planes, np_dtype)
        assert same_bits(got, want), (dtype, int((got != want).sum()))


def test_finish_into_a_separate_float_buffer_and_without_an_accumulator():
    dims = (3, 4, 2)
    planes = random_planes(dims, seed=5)
    full = tuple(2 * d for d in dims)
    acc = torch.empty(full, dtype=torch.float32, device="cuda")
    out = torch.empty(full, dtype=torch.float32, device="cuda")
    up2_blend(slice_major(planes[1], 1), 1, acc, L.VOLBLEND_SET)
    before = acc.clone()
    up2_blend(slice_major(planes[2], 2), 2, acc, L.VOLBLEND_FINISH, 2, out)
    assert same_bits(out.cpu().numpy(), combine_planes_np({1: planes[1], 2: planes[2]}))
    assert torch.equal(acc, before)                             # FINISH writes out only
    assert same_bits(before.cpu().numpy(), combine_planes_np({1: planes[1]}))
    alone = torch.empty(full, dtype=torch.int16, device="cuda")
    up2_blend(slice_major(planes[0], 0), 0, None, L.VOLBLEND_FINISH, 1, alone)
    assert same_bits(alone.cpu().numpy(), combine_planes_np({0: planes[0]}, np.int16))


def test_int16_ties_and_saturation_on_the_device():
    """Multiples of 4 up to +-60000: 0.75 e and 0.25 e are integers, so the mean of two planes is an integer or a tie, and a
    part of the values lies past the int16 range."""
    dims = (5, 6, 7)
    planes = random_planes(dims, seed=11, scale=60000.0, step=4.0)
    two = {0: planes[0], 1: planes[1]}
    mean = combine_planes_np(two)
    assert (mean - np.floor(mean) == 0.5).any() and (np.abs(mean) > 32768).any()
    assert same_bits(run_blend(two, dims, torch.int16), combine_planes_np(two, np.int16))
    assert same_bits(run_blend(planes, dims, torch.int16), combine_planes_np(planes, np.int16))


def test_refusals_return_their_code_without_a_launch():
    lib = L.load()
    plane = torch.zeros((2, 4, 4), dtype=torch.float32, device="cuda")
    acc = torch.full((4, 4, 4), 7.0, dtype=torch.float32, device="cuda")
    out = torch.full((4, 4, 4), 9.0, dtype=torch.float32, device="cuda")
    p, a, o, st = plane.data_ptr(), acc.data_ptr(), out.data_ptr(), L.stream_ptr()

    def call(plane=p, axis=0, X=2, Y=2, Z=2, acc=a, mode=L.VOLBLEND_FINISH, count=3, out_dtype=L.WINDOW_F32, out=o):
        return lib.mrisr_f32_volume_up2_blend(plane, axis, X, Y, Z, acc, mode, count, out_dtype, out, st)

    assert call(plane=None) == E_ARG and b"null" in lib.mrisr_last_error()
    assert call(acc=None) == E_ARG and call(acc=None, mode=L.VOLBLEND_SET) == E_ARG and call(out=None) == E_ARG
    assert call(axis=3) == E_ARG and call(axis=-1) == E_ARG
    assert call(mode=3) == E_ARG and call(mode=-1) == E_ARG
    assert call(out_dtype=2) == E_ARG and call(count=0) == E_ARG
    assert call(plane=p + 4, axis=1) == E_ARG                   # a float buffer off the 8-byte boundary
    assert call(X=0) == E_SHAPE and call(Y=-1) == E_SHAPE and call(Z=0) == E_SHAPE
    assert call(X=32768) == E_SHAPE and call(axis=2, Z=32768) == E_SHAPE
    assert call(axis=0, Y=32767, Z=32767) == E_SHAPE            # a doubled slice past the 32-bit row index of the stream form
    torch.cuda.synchronize()
    assert (acc == 7.0).all() and (out == 9.0).all()            # nothing was launched
    with pytest.raises(ValueError):
        up2_blend(plane.transpose(1, 2), 0, acc, L.VOLBLEND_SET)      # not contiguous
    with pytest.raises(ValueError):
        up2_blend(plane, 0, acc[:2], L.VOLBLEND_SET)                  # (2, 4, 4) across axis 0 fills a (4, 4, 4) accumulator
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        up2_blend(plane.cpu(), 0, acc, L.VOLBLEND_SET)


# ---------------------------------------------------------------- end to end

def synthetic_volume(shape, seed=0, constant_slice=CONSTANT_SLICE):
    """The generator of tests/test_gpu_volume.py: intensities 0..3000, smooth structure plus noise, a dark background of exact
    zeros; one constant slice across axis 2."""
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*(np.linspace(-1, 1, s) for s in shape), indexing="ij")
    v = 3000.0 * np.exp(-2.0 * (x * x + y * y)) * (0.6 + 0.4 * np.cos(3 * x + z)) + rng.normal(0, 40, shape)
    v = np.clip(np.rint(v), 0, 3000)
    v[:3] = 0
    if constant_slice is not None:
        v[:, :, constant_slice] = CONSTANT_VALUE
    return v.astype(np.float32)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(1234)
    m = UNetSuperRes(1, 1, base_filters=16)
    return m.cuda().eval()


def eager_planes(model, vol):
    x = torch.from_numpy(vol).cuda()
    return {a: enhance_volume(model, x, axis=a, batch_size=2, use_graph=False).cpu().numpy() for a in (0, 1, 2)}


@pytest.fixture(scope="module")
def case(model):
    """The volume, its three eager enhance_volume passes and their combination: computed once, read by every test below."""
    vol = synthetic_volume((24, 40, 32))
    planes = eager_planes(model, vol)
    return vol, planes, combine_planes_np(planes)


def slice_windows(vol, axis):
    """hi - lo of every slice across axis."""
    moved = np.moveaxis(vol, axis, 0)
    lohi = np.stack([imageops.percentile_bounds_np(np.ascontiguousarray(s)) for s in moved])
    return (lohi[:, 1] - lohi[:, 0]).astype(np.float64)


def test_isotropic_eager_is_bit_equal_to_the_combined_passes(model, case):
    vol, planes, want = case
    assert [planes[a].shape for a in (0, 1, 2)] == [(24, 80, 64), (48, 40, 64), (48, 80, 32)]
    out = enhance_volume_isotropic(model, torch.from_numpy(vol).cuda(), batch_size=2, use_graph=False)
    assert tuple(out.shape) == (48, 80, 64) and out.dtype == torch.float32 and out.is_contiguous()
    assert same_bits(out.cpu().numpy(), want)
    # not a comparison between clamped constants: some output slice spans more than 5 % of its input slice's window
    got, win = out.cpu().numpy(), slice_windows(vol, 2)
    spans = [(got[:, :, z].max() - got[:, :, z].min()) / win[z // 2] for z in range(64) if win[z // 2] > 0]
    print(f"largest span of an output slice: {max(spans):.3f} of its window")
    assert max(spans) > 0.05
    i16 = enhance_volume_isotropic(model, torch.from_numpy(vol).cuda(), batch_size=2, use_graph=False, out_dtype=torch.int16)
    assert i16.dtype == torch.int16 and same_bits(i16.cpu().numpy(), combine_planes_np(planes, np.int16))
    sub = enhance_volume_isotropic(model, torch.from_numpy(vol).cuda(), planes=(2, 0), batch_size=2, use_graph=False)
    assert same_bits(sub.cpu().numpy(), combine_planes_np({0: planes[0], 2: planes[2]}))


def test_isotropic_graph_is_within_the_bar_of_the_eager_result(model, case):
    vol, _, want = case
    out = enhance_volume_isotropic(model, torch.from_numpy(vol).cuda(), batch_size=2, use_graph=True).cpu().numpy()
    bound = np.zeros(want.shape)
    for a in (0, 1, 2):
        w = slice_windows(vol, a)
        widest = np.maximum(w, np.maximum(np.concatenate([w[:1], w[:-1]]), np.concatenate([w[1:], w[-1:]])))      # s - 1, s, s + 1
        shape = [1, 1, 1]
        shape[a] = -1
        bound = bound + np.repeat(widest, 2).reshape(shape) / 3.0
    err = np.abs(out.astype(np.float64) - want)
    print(f"graph against eager: max error {err.max():.3e} intensity units, largest share of its bar {(err / (BAR * bound + 1e-3)).max():.3e}")
    assert (err <= BAR * bound + 4 * np.spacing(np.float32(3000.0))).all()


def test_odd_sized_volume_through_the_transposing_form(model):
    vol = synthetic_volume((25, 35, 3), seed=3, constant_slice=None)
    x = torch.from_numpy(vol).cuda()
    out = enhance_volume_isotropic(model, x, planes=(2,), batch_size=2, use_graph=False)
    assert tuple(out.shape) == (50, 70, 6)
    want = combine_planes_np({2: enhance_volume(model, x, axis=2, batch_size=2, use_graph=False).cpu().numpy()})
    assert same_bits(out.cpu().numpy(), want)


def test_refusals_of_the_python_entry(model, case):
    vol, _, _ = case
    x = torch.from_numpy(vol).cuda()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enhance_volume_isotropic(model, torch.from_numpy(vol))
    for bad in ((), (0, 0), (3,), (0, 1, 2, 2)):
        with pytest.raises(ValueError):
            enhance_volume_isotropic(model, x, planes=bad)
    with pytest.raises(ValueError):
        enhance_volume_isotropic(model, x[0])
    with pytest.raises(ValueError):
        enhance_volume_isotropic(model, x.double())
    with pytest.raises(ValueError):
        enhance_volume_isotropic(model, x, out_dtype=torch.uint8)
    with pytest.raises(ValueError):
        enhance_volume_isotropic(model, x, batch_size=0)


def test_command_line(model, case, tmp_path):
    vol, planes, want = case
    ckdir = tmp_path / "ck"
    ckdir.mkdir()
    torch.save({"model_state_dict": {k: v.cpu() for k, v in model.state_dict().items()}}, ckdir / "best_model_unet.pth")
    affine = np.array([[0.9, 0.0, 0.1, -20.0], [0.0, 1.1, 0.0, 30.0], [-0.1, 0.0, 3.0, 5.0], [0, 0, 0, 1]])
    src = tmp_path / "scan.nii.gz"
    write_nifti(str(src), vol, NiftiHeader.new(vol.shape, (0.9, 1.1, 3.0), affine), ())
    common = ["--checkpoint_dir", str(ckdir), "--base_filters", "16", "--batch_size", "2"]

    def run(*argv):
        return infer_volume.main(infer_volume.parse_args(list(argv) + common))

    out_path = tmp_path / "out" / "iso.nii.gz"
    assert run("--input", str(src), "--output", str(out_path), "--isotropic") == 0            # default: graph replay
    data, hdr = read_nifti(str(out_path))
    graph = enhance_volume_isotropic(model, torch.from_numpy(vol).cuda(), batch_size=2).cpu().numpy()
    assert data.shape == (48, 80, 64) and hdr.get("datatype") == 16 and hdr.get("dim")[:4] == [3, 48, 80, 64]
    assert np.array_equal(data, graph)
    assert hdr.get("pixdim")[1:4] == pytest.approx([0.45, 0.55, 1.5])
    centre_in = affine @ np.array([11.5, 19.5, 15.5, 1.0])          # the volume's centre stays where it was
    assert np.allclose(hdr.affine() @ np.array([23.5, 39.5, 31.5, 1.0]), centre_in, atol=1e-4)

    i16_path = tmp_path / "i16.nii"
    assert run("--input", str(src), "--output", str(i16_path), "--isotropic", "--output_dtype", "int16", "--no_graph", "--axis", "0") == 0
    data16, hdr16 = read_nifti(str(i16_path))
    assert hdr16.get("datatype") == 4 and hdr16.get("bitpix") == 16
    assert np.array_equal(data16, combine_planes_np(planes, np.int16).astype(np.float32))      # --axis is not used

    src4 = tmp_path / "scan4d.nii.gz"
    vol4 = np.stack([vol, vol[::-1].copy()], axis=3)
    write_nifti(str(src4), vol4, NiftiHeader.new(vol4.shape, (0.9, 1.1, 3.0, 2.0), affine), ())
    out4 = tmp_path / "out4d.nii.gz"
    assert run("--input", str(src4), "--output", str(out4), "--isotropic", "--no_graph") == 0
    data4, hdr4 = read_nifti(str(out4))
    assert data4.shape == (48, 80, 64, 2) and hdr4.get("dim")[:5] == [4, 48, 80, 64, 2]
    assert hdr4.get("pixdim")[1:5] == pytest.approx([0.45, 0.55, 1.5, 2.0])
    assert np.allclose(hdr4.affine() @ np.array([23.5, 39.5, 31.5, 1.0]), centre_in, atol=1e-4)
    assert np.array_equal(data4[..., 0], want)
    second = enhance_volume_isotropic(model, torch.from_numpy(vol4[..., 1].copy()).cuda(), batch_size=2, use_graph=False)
    assert np.array_equal(data4[..., 1], second.cpu().numpy())

    plain = tmp_path / "plain.nii"
    assert run("--input", str(src), "--output", str(plain), "--no_graph") == 0               # without the flag: as before
    assert np.array_equal(read_nifti(str(plain))[0], planes[2])
