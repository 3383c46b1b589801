"""The ABI listing of the three head_dim-72 attention entry points (csrc/attention_d72.hip): header, lib.SYMBOLS and, when it is built, the library."""
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_abi_lists_the_three_d72_attention_symbols():
    from simpletuner_amd import lib
    header = (ROOT / "include" / "st355.h").read_text()
    for n in ("st355_attn_d72_fwd", "st355_attn_d72_bwd", "st355_attn_d72_bwd_workspace"):
        assert n in lib.SYMBOLS and f"{n}(" in header, n
    if Path(lib.LIB_PATH).exists():
        assert all(hasattr(lib.load(), n) for n in lib.SYMBOLS if "attn_d72" in n)
