"""training.optimizer.flat_view: the one place that turns a list of back-to-back tensor views into the 1-D view over their arena."""
import pytest
import torch

from simpletuner_amd.training.optimizer import flat_view

SHAPES = [(8, 16), (16, 8), (8, 8)]


def _views(buf, shapes=SHAPES, gap=0):
    out, off = [], 0
    for s in shapes:
        k = s[0] * s[1]
        out.append(buf[off:off + k].view(s))
        off += k + gap
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_back_to_back_views_give_one_view_over_the_arena(dtype):
    buf = torch.arange(400, dtype=torch.float32).to(dtype)
    ts = _views(buf[16:])                                        # the run need not start at the allocation's first element
    flat = flat_view(ts)
    assert flat is not None and flat.dim() == 1 and flat.dtype == dtype
    assert flat.numel() == sum(t.numel() for t in ts) == 320
    assert flat.data_ptr() == ts[0].data_ptr() and flat.untyped_storage().data_ptr() == ts[0].untyped_storage().data_ptr()
    assert torch.equal(flat, buf[16:336])
    before = buf.clone()
    flat.fill_(7.0)                                              # writes through the view land in the tensors
    assert all(bool((t == 7.0).all()) for t in ts)
    assert torch.equal(buf[:16], before[:16]) and torch.equal(buf[336:], before[336:])       # and nowhere else
    ts[1][3, 2] = -1.0                                           # and the other way round
    assert flat[128 + 3 * 8 + 2] == -1.0
    assert flat_view(ts[:1]).numel() == 128


def test_what_is_not_one_run_gives_none():
    buf = torch.zeros(400)
    ts = _views(buf)
    assert flat_view([]) is None
    assert flat_view([ts[0], None, ts[2]]) is None
    assert flat_view([None]) is None
    mid = buf[128:192].view(torch.bfloat16).view(16, 8)                                      # the bytes right behind ts[0], as bf16
    assert mid.data_ptr() == ts[0].data_ptr() + 512 and buf[192:256].data_ptr() == mid.data_ptr() + 256
    assert flat_view([ts[0], mid, buf[192:256].view(8, 8)]) is None                          # mixed dtypes, back to back in memory
    assert flat_view(_views(buf, SHAPES[:2], gap=1)) is None                                 # a gap of one element
    assert flat_view([ts[1], ts[0], ts[2]]) is None                                          # swapped order
    assert flat_view([ts[0], buf[128:256].view(8, 16).t(), ts[2]]) is None                   # a transposed member: same bytes, not contiguous
    assert flat_view(ts) is not None
