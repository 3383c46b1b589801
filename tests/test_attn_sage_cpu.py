"""attention_mechanism=sageattention off the GPU: the ABI listing of the three entry points (csrc/attention_sage.hip), the config parsing with its refusals by
name, and the SD3 sampling forward on the emulator with the option absent (the stream of ops calls is the one of a config that never heard of the option; the
flag-off launch stream itself is pinned against the recorded digests by tests/test_dora_cpu.py and its kin, which run the same host-sequencing forward)."""
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from tests import ops_emulator as EMU
from tests.test_sd3_host_sequencing_cpu import _arch
from tests.test_self_transcendence_cpu import _trace

ROOT = Path(__file__).resolve().parent.parent
BF16 = torch.bfloat16


def test_abi_lists_the_three_sage_attention_symbols():
    from simpletuner_amd import lib
    header = (ROOT / "include" / "st355.h").read_text()
    for n in ("st355_attn_sage_workspace", "st355_attn_sage_quantize", "st355_attn_sage_fwd"):
        assert n in lib.SYMBOLS and f"{n}(" in header, n
    if Path(lib.LIB_PATH).exists():
        assert all(hasattr(lib.load(), n) for n in lib.SYMBOLS if "attn_sage" in n)


@pytest.mark.parametrize("mech,usage,want", [(None, None, False), ("diffusers", "training", False), ("sla", None, False), ("sageattention", None, True),
                                             ("sageattention", "", True), ("SageAttention-int8-fp8-cuda", "Inference", True), ("sageattention", "None", True)])
def test_config_parsing(mech, usage, want):
    from simpletuner_amd.engine import sage_attention_enabled
    cfg = SimpleNamespace(**{k: v for k, v in (("attention_mechanism", mech), ("sageattention_usage", usage)) if v is not None})
    assert sage_attention_enabled(cfg) is want


@pytest.mark.parametrize("mech,usage,exc,msg", [("sageattention", "training", NotImplementedError, "sageattention_usage=training"),
                                                ("sageattention", "training+inference", NotImplementedError, r"sageattention_usage=training\+inference"),
                                                ("sageattention-int8-fp16-cuda", None, NotImplementedError, "attention_mechanism=sageattention-int8-fp16-cuda"),
                                                ("sageattention-int8-fp16-triton", "inference", NotImplementedError, "attention_mechanism=sageattention-int8-fp16-triton"),
                                                ("sageattention", "sometimes", ValueError, "Unsupported attention backend mode 'sometimes'")])
def test_what_is_not_built_is_refused_by_name(mech, usage, exc, msg):
    from simpletuner_amd.engine import sage_attention_enabled
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import default_config
    with pytest.raises(exc, match=msg):
        sage_attention_enabled(SimpleNamespace(attention_mechanism=mech, sageattention_usage=usage))
    cfg = default_config(model_family="sd3")
    cfg.attention_mechanism, cfg.sageattention_usage = mech, usage
    with pytest.raises(exc, match=msg):          # and at the plugin's config check, before any step
        SD3(cfg, SimpleNamespace(device=torch.device("cpu"), num_processes=1, process_index=0, is_main_process=True)).check_user_config()


def test_sd3_sampling_with_the_option_absent_launches_what_it_always_launched(monkeypatch):
    EMU.install(monkeypatch)
    from simpletuner_amd.sampling import sample_images
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import default_config
    acc = SimpleNamespace(device=torch.device("cpu"), num_processes=1, process_index=0, is_main_process=True)
    plugin = SD3(default_config(model_family="sd3", lora_rank=8, train_batch_size=1, seed=3, lora_init_b_std=0.02, flow_schedule_shift=3.0), acc)
    plugin.load_model(**_arch(2, qk_norm="rms_norm", dual=(0,)))
    plugin.add_lora_adapter()
    model = plugin.get_trained_component()
    g = torch.Generator().manual_seed(2)
    pe, pool, x0 = torch.randn(1, 20, 128, generator=g).to(BF16), torch.randn(1, 64, generator=g).to(BF16), torch.randn(1, 16, 16, 16, generator=g).to(BF16)
    outs = []

    def run():
        with torch.no_grad():
            outs.append(sample_images(plugin, pe, pool, 16, 16, num_inference_steps=2, decode=False, latents=x0.clone()))

    assert not hasattr(plugin.config, "attention_mechanism") or plugin.config.attention_mechanism is None
    with monkeypatch.context() as mp:
        absent = _trace(mp, run)
    plugin.config.attention_mechanism = "diffusers"          # any other value changes nothing either
    with monkeypatch.context() as mp:
        other = _trace(mp, run)
    assert absent == other and torch.equal(*outs) and model._sage_eval is False
    # block 0 is a dual block (host sequencing: joint + image-only attention), block 1 goes through its C entry point, which the emulator counts on its own
    assert absent.count("attn_fwd") == 2 * 2 and not any(n.startswith("attn_sage") for n in absent), absent
    plugin.config.attention_mechanism = "sageattention"      # set: the phase is entered (the emulator has no quantised kernel, so the first attention says so)
    from simpletuner_amd import lib
    with pytest.raises((lib.St355Error, RuntimeError, AttributeError)):
        run()
    assert model._sage_eval is False                         # and left again on the way out
