"""ops._scratch: the one device-scratch helper and its one growth rule (grow-only, an outgrown buffer is retired, growth inside a hipGraph capture is
refused).  Host logic only: driven with CPU devices, torch.cuda.is_current_stream_capturing patched."""
import inspect
import re

import pytest
import torch

from simpletuner_amd import ops
from simpletuner_amd.lib import St355Error

CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def _fresh_table(monkeypatch):
    monkeypatch.setattr(ops, "_scratch_bufs", {})
    monkeypatch.setattr(ops, "_scratch_retired", [])


def _capturing(monkeypatch, value):
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: value)


def _no_query(monkeypatch):
    def boom():
        raise RuntimeError("is_current_stream_capturing was queried")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", boom)


def test_first_request_allocates_the_bytes_asked_for(monkeypatch):
    _no_query(monkeypatch)                      # a first allocation never asks about captures either
    ws = ops._scratch("a", CPU, 1000)
    assert ws.dtype == torch.uint8 and ws.numel() >= 1000 and ws.device == CPU
    assert ops._scratch_retired == []


def test_equal_or_smaller_request_returns_the_same_buffer(monkeypatch):
    _capturing(monkeypatch, False)
    ws = ops._scratch("a", CPU, 1000)
    for n in (1000, 999, 1, 0):
        again = ops._scratch("a", CPU, n)
        assert again is ws and again.data_ptr() == ws.data_ptr() and again.numel() == ws.numel()
    assert ops._scratch_retired == []


def test_larger_request_retires_the_old_buffer(monkeypatch):
    _capturing(monkeypatch, False)
    old = ops._scratch("a", CPU, 1000)
    new = ops._scratch("a", CPU, 1001)
    assert new is not old and new.data_ptr() != old.data_ptr() and new.numel() >= 1001
    assert len(ops._scratch_retired) == 1 and ops._scratch_retired[0] is old
    assert ops._scratch("a", CPU, 1000) is new          # grow-only: the smaller request now gets the grown buffer


def test_capture_allows_a_first_allocation_and_refuses_growth(monkeypatch):
    _capturing(monkeypatch, True)
    old = ops._scratch("a", CPU, 1000)
    assert old.numel() >= 1000
    with pytest.raises(St355Error, match="hipGraph capture") as e:
        ops._scratch("a", CPU, 2000)
    msg = str(e.value)
    assert "the a scratch" in msg and "1000" in msg and "2000" in msg
    assert msg.endswith("inside a hipGraph capture: run one eager step first")
    assert ops._scratch_retired == []
    assert len(ops._scratch_bufs) == 1 and ops._scratch("a", CPU, 1000) is old


def test_capture_query_sits_on_the_growth_path_only(monkeypatch):
    _capturing(monkeypatch, False)
    ws = ops._scratch("a", CPU, 1000)
    _no_query(monkeypatch)
    assert ops._scratch("a", CPU, 1000) is ws and ops._scratch("a", CPU, 10) is ws
    with pytest.raises(RuntimeError, match="was queried"):
        ops._scratch("a", CPU, 1001)


def test_names_and_keys_never_alias(monkeypatch):
    _capturing(monkeypatch, False)
    bufs = [ops._scratch("a", CPU, 64), ops._scratch("b", CPU, 64), ops._scratch("a", CPU, 64, key=(1,)), ops._scratch("a", CPU, 64, key=(2,)),
            ops._scratch("b", CPU, 64, key=(1,))]
    assert len({b.data_ptr() for b in bufs}) == len(bufs) and len(ops._scratch_bufs) == len(bufs)
    assert ops._scratch("a", CPU, 64, key=(1,)) is bufs[2] and ops._scratch("a", CPU, 64) is bufs[0]
    grown = ops._scratch("a", CPU, 128, key=(1,))         # growing one leaves the others where they are
    assert len(ops._scratch_retired) == 1 and ops._scratch_retired[0] is bufs[2]
    assert grown is not bufs[2] and ops._scratch("a", CPU, 64, key=(2,)) is bufs[3] and ops._scratch("a", CPU, 64) is bufs[0]


def test_the_gemm_workspace_is_one_fixed_size(monkeypatch):
    seen = []
    monkeypatch.setattr(ops, "_scratch", lambda name, dev, nbytes, key=(): seen.append((name, dev, nbytes, key)) or "buf")
    assert ops._gemm_workspace(CPU) == "buf" and seen == [("gemm", CPU, 512 << 20, ())]


def test_ops_keeps_no_scratch_dict_of_its_own():
    """every wrapper takes its scratch from _scratch: no module-level `_*_ws = {}` and exactly one retired list"""
    src = inspect.getsource(ops)
    assert re.findall(r"^_\w*_ws\s*=\s*\{\}", src, flags=re.M) == []
    assert re.findall(r"^(\w*retired\w*)\s*=", src, flags=re.M) == ["_scratch_retired"]
