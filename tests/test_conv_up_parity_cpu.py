"""Host side of the nearest-2x parity form (``lfvdm_conv_args::up = 3``): which argument records get tune codes, the A/B
switch, and the plumbing of ``lfvdm_pack_conv_weight_up2x``.  ``lfvdm_conv_igemm_candidates`` launches nothing, so this
runs without a GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000      # stands in for device pointers: the query never dereferences them


def args(nat, **kw):
    a = nat.ConvArgs()
    a.src0, a.W, a.out = FAKE, FAKE, FAKE
    a.N, a.Hs, a.Ws, a.C0, a.Cout = 2, 8, 8, 128, 128
    a.Ho, a.Wo, a.ksize, a.stride, a.up = 16, 16, 3, 1, 3
    a.ldo = a.ldr = 128
    a.out_mode = nat.OUT_ROWS
    a.splitk_ws, a.splitk_cnt, a.splitk_ws_floats, a.splitk_cnt_ints = FAKE, FAKE, 2 * 1024 * 1024, 4096
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def count(nat, a):
    codes = (C.c_int * 256)()
    return nat.lib().lfvdm_conv_igemm_candidates(C.byref(a), codes, 256), codes


def test_export_is_declared_and_bound():
    from improved_diffusion import _native
    hdr = open(os.path.join(ROOT, "include", "lfvdm_hip.h")).read()
    assert re.search(r"\blfvdm_pack_conv_weight_up2x\s*\(", hdr)
    assert "lfvdm_pack_conv_weight_up2x" in _native.EXPORTS and len(_native._SIGS["lfvdm_pack_conv_weight_up2x"][0]) == 5
    lib = C.CDLL(_native.LIB_PATH)
    assert hasattr(lib, "lfvdm_pack_conv_weight_up2x")
    assert lib.lfvdm_abi_version() == 9


def test_codes_exist_exactly_for_the_legal_form(monkeypatch):
    from improved_diffusion import _native as nat
    monkeypatch.delenv("LFVDM_CONV_NO_UP_PARITY", raising=False)
    n, codes = count(nat, args(nat))
    assert n > 0
    assert any(((codes[i] - 1) >> 5) & 7 for i in range(n)), "split-K codes are offered with a workspace"
    assert not any((((codes[i] - 1) >> 5) & 7) == 4 for i in range(n)), "no tail split in the class form"
    assert count(nat, args(nat, res=FAKE, bias=FAKE))[0] > 0
    # K = 4 * Cin: a tile with four k-groups needs at least four 32-channel chunks - one 32-channel source has exactly four
    assert count(nat, args(nat, C0=32, Cout=32, ldo=32, ldr=32))[0] > 0
    refused = dict(concat=dict(C1=128, src1=FAKE), skip=dict(s2C0=128, s2src0=FAKE, W2=FAKE),
                   gn_out=dict(gn_out=FAKE, gn_gamma=FAKE, gn_beta=FAKE, gn_film_div=1), resA=dict(res=FAKE, resA=FAKE, resB=FAKE),
                   nchw=dict(out_mode=nat.OUT_NCHW), stride=dict(stride=2, Ho=8, Wo=8), k1=dict(ksize=1, Ho=16, Wo=16))
    for name, kw in refused.items():
        assert count(nat, args(nat, **kw))[0] == 0, name
    # the nine-tap form of the same launch keeps its codes
    assert count(nat, args(nat, up=1))[0] > 0


def test_switch_refuses_the_form_per_call(monkeypatch):
    from improved_diffusion import _native as nat
    monkeypatch.setenv("LFVDM_CONV_NO_UP_PARITY", "1")
    assert count(nat, args(nat))[0] == 0
    assert count(nat, args(nat, up=1))[0] > 0
    monkeypatch.delenv("LFVDM_CONV_NO_UP_PARITY")
    assert count(nat, args(nat))[0] > 0
