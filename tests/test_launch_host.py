"""mri_superresolution_amd/launch.py on the CPU: what the shared helpers put into the C structs (CPU tensors' data_ptr() serve as
addresses; nothing is launched)."""
import pytest
import torch

from mri_superresolution_amd import _lib as L
from mri_superresolution_amd.launch import Consumer, dgrad_desc, marshal_consumers

HEAD_FIELDS = ("head_out", "head_w", "head_part", "head_dw", "head_db")


def _buf():
    return torch.zeros(4)


def test_consumer_fields_land_in_the_struct_field_of_the_same_name():
    head = tuple(_buf() for _ in HEAD_FIELDS)
    k = Consumer(da=_buf(), C_total=11, c_off=12, H=13, W=14, spatial=L.SP_HEAD, off_y=15, off_x=16, weight_mode=2, head=head)
    ints = ("C_total", "c_off", "H", "W", "spatial", "off_y", "off_x", "weight_mode")
    assert len({getattr(k, f) for f in ints}) == len(ints)                  # a distinct value in every field
    assert len({k.da.data_ptr(), *(t.data_ptr() for t in head)}) == 6
    c = marshal_consumers([k])[0]
    assert c.da == k.da.data_ptr()
    for f in ints:
        assert getattr(c, f) == getattr(k, f), f
    for f, t in zip(HEAD_FIELDS, head):
        assert getattr(c, f) == t.data_ptr(), f


def test_consumer_without_head_has_null_head_pointers_and_two_fill_both_slots():
    a, b = Consumer(_buf(), 8, 0, 5, 6, L.SP_NONE, 0, 0), Consumer(_buf(), 24, 8, 5, 6, L.SP_POOL2, 1, 2)
    cons = marshal_consumers([a, b])
    assert len(cons) == 2
    for c, k in zip(cons, (a, b)):
        assert c.da == k.da.data_ptr() and (c.C_total, c.c_off, c.spatial) == (k.C_total, k.c_off, k.spatial)
        assert c.weight_mode == 0
        assert all(getattr(c, f) is None for f in HEAD_FIELDS)


@pytest.mark.parametrize("count", [0, 3])
def test_only_one_or_two_consumers_marshal(count):
    with pytest.raises(RuntimeError):
        marshal_consumers([Consumer(_buf(), 8, 0, 5, 6, L.SP_NONE, 0, 0) for _ in range(count)])


def test_dgrad_descriptor_mirrors_the_forward_layer():
    a, b, n, h, w = 24, 40, 2, 5, 7                                         # forward layer: Cin = a, Cout = b
    dy, out, wp, ring = torch.zeros(n, h, w, b), torch.zeros(n, h, w, a), _buf(), _buf()
    d = dgrad_desc(L.BF16, dy, a, b, 3, wp, out, ring, cu_limit=152)
    assert (d.dtype, d.N, d.H, d.W, d.ksize) == (L.BF16, n, h, w, 3)
    assert (d.Cin, d.Cout, d.nsrc) == (b, a, 1)
    s = d.src[0]
    assert (s.ptr, s.C, s.H, s.W) == (dy.data_ptr(), b, h, w)
    assert (s.mode, s.spatial, s.off_y, s.off_x) == (L.SRC_RAW, L.SP_NONE, 0, 0)
    assert s.scale is None and s.shift is None
    assert (d.combine, d.out_mode, d.groups, d.relu_out) == (L.COMBINE_CONCAT, L.OUT_PLAIN, 0, 0)
    assert (d.wpacked, d.wpacked_ring, d.out, d.cu_limit) == (wp.data_ptr(), ring.data_ptr(), out.data_ptr(), 152)
    assert d.bias is None and d.stats is None and d.relu_mask is None and d.blend_alpha is None
    plain = dgrad_desc(L.F32, dy, a, b, 3, wp, out)                          # the blocks and the VGG stack: no ring image, whole chip
    assert plain.wpacked_ring is None and plain.cu_limit == 0
