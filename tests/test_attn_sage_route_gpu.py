"""attention_mechanism=sageattention on the tiny SD3 / SD3.5 and Flux models: `sample_images` runs every attention of every forward on ops.attn_sage_fwd and
none on ops.attn_fwd (SD3.5's image-only attention included), a train step under the same config is bit-identical to one without the option, and the sampled
latents are finite.  No closeness threshold here: the accuracy of the quantised forward is pinned at the kernel (tests/test_attn_sage_gpu.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
STEPS = 2


def _count(monkeypatch, ops):
    calls = {"attn_sage_fwd": 0, "attn_fwd": 0}
    for n in calls:
        monkeypatch.setattr(ops, n, lambda *a, _f=getattr(ops, n), _n=n, **k: (calls.__setitem__(_n, calls[_n] + 1), _f(*a, **k))[1])
    return calls


@pytest.mark.parametrize("family", ["sd3", "sd35", "flux"])
def test_sampling_takes_the_quantised_route_and_training_does_not(monkeypatch, family):
    from simpletuner_amd import ops
    from simpletuner_amd.sampling import sample_images
    if family == "flux":
        from tests.test_flux_model_gpu import _batch, _build
        build = lambda: _build(1, 2, 1, 16, 16, 40)
        attns = 1 + 2                                                   # one double block, two single blocks
    else:
        from tests.test_sd3_model_gpu import _batch, _build
        build = lambda: _build(2, 1, 16, 16, 40, **(dict(qk_norm="rms_norm", dual=(0,)) if family == "sd35" else {}))
        attns = 2 + (family == "sd35")                                  # SD3.5: block 0 also runs the image-only attention
    state = []
    for mech in (None, "sageattention"):
        plugin, trainer, _cpu, devt = build()
        plugin.sample_flow_sigmas = lambda batch, state, sig=devt["sigmas"]: (sig, sig * 1000.0)          # the same timesteps in both builds
        if mech:
            plugin.config.attention_mechanism = mech
            plugin.check_user_config()
        loss = trainer.train_step(dict(_batch(devt)))
        state.append((loss.detach().clone(), plugin.get_trained_component().lora_flat.clone()))
    assert torch.equal(state[0][0], state[1][0]) and torch.equal(state[0][1], state[1][1]), "the option changed a train step"
    calls = _count(monkeypatch, ops)
    with torch.no_grad():
        x = sample_images(plugin, devt["prompt"], devt["pooled"], 16, 16, num_inference_steps=STEPS, decode=False, generator=torch.Generator(device="cuda:0").manual_seed(1))
    assert calls == {"attn_sage_fwd": attns * STEPS, "attn_fwd": 0}, calls
    assert bool(torch.isfinite(x.float()).all())
    calls.update(attn_sage_fwd=0, attn_fwd=0)
    trainer.train_step(dict(_batch(devt)))                              # after sampling: training is back on the exact kernels (or on the C block entry points)
    assert calls["attn_sage_fwd"] == 0
