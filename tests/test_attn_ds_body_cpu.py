"""The dS-spill variant of the dK / dV body (tools/kgen/dkv.py, DKV_DS=1 -> simpletuner_amd/csrc/gen/attn_dkv4_ds_body.inc): the generator reproduces the committed
file byte for byte and passes its own checks on the way (counted LDS waits with the loop back-edge assertion, the gfx950 hazard table including the wide-store ->
data-register-overwrite rule); with default options it still emits attn_dkv4_body.inc; and the variant IS the default stream plus the spill — the same
instructions in the same order once the stores, their base's scalar adds and the counted tile wait are taken out."""
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
GEN = ROOT / "simpletuner_amd" / "csrc" / "gen"


def _generate(tmp_path, name, **env_extra):
    out = tmp_path / name
    env = {k: v for k, v in os.environ.items() if not k.startswith(("FWD64_", "DQ64_", "DKV_"))}
    env.update({"DKV_OUT": str(out), **env_extra})
    r = subprocess.run([sys.executable, "-m", "tools.kgen.dkv"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_bytes()


def test_ds_generator_reproduces_the_committed_body(tmp_path):
    assert _generate(tmp_path, "attn_dkv4_ds_body.inc", DKV_DS="1") == (GEN / "attn_dkv4_ds_body.inc").read_bytes()
    assert not (tmp_path / "attn_dkv4_clobbers.inc").exists()          # the variant owns the same registers: no clobber list of its own


def test_default_options_still_reproduce_the_default_body(tmp_path):
    assert _generate(tmp_path, "attn_dkv4_body.inc") == (GEN / "attn_dkv4_body.inc").read_bytes()
    assert _generate(tmp_path, "attn_dkv4_body0.inc", DKV_DS="0") == (GEN / "attn_dkv4_body.inc").read_bytes()


def test_ds_body_is_the_default_stream_plus_the_spill():
    ds = (GEN / "attn_dkv4_ds_body.inc").read_text().splitlines()
    base = (GEN / "attn_dkv4_body.inc").read_text().splitlines()
    stores = [ln for ln in ds if "global_store_dwordx4" in ln]
    # every 32-query block of the unrolled stream (16 exponentials each) spills through two stores
    blocks = sum(1 for ln in base if "v_exp_f32" in ln) // 16
    assert len(stores) == 2 * blocks and all("%[dsoff]" in ln and "s[56:57]" in ln for ln in stores)
    assert sorted({ln.split("offset:")[1].split("\\")[0].strip() for ln in stores}) == ["0", "1024", "2048", "3072"]
    spill = ("global_store_dwordx4", "s_add_u32 s56", "s_addc_u32 s57", "%[dsbase]")
    kept = [ln for ln in ds if not any(t in ln for t in spill)]
    kept = [ln.replace("s_waitcnt vmcnt(2)", "s_waitcnt vmcnt(0)") for ln in kept]
    assert kept == base


def test_wide_store_hazard_is_enforced():
    from tools.kgen.emit import check_hazards

    bad = check_hazards(["global_store_dwordx4 v1, v[112:115], s[56:57] offset:0", "v_mov_b32_e32 v113, 0"])
    assert bad and "needs 2 states" in bad[0]
    assert not check_hazards(["global_store_dwordx4 v1, v[112:115], s[56:57] offset:0", "s_nop 1", "v_mov_b32_e32 v113, 0"])
    assert not check_hazards(["global_store_dwordx2 v1, v[112:113], s[56:57]", "v_mov_b32_e32 v113, 0"])
