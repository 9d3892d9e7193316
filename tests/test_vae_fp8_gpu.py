"""VaeEngine.fp8_conv (r19): the ResidualBlock convolutions of the VAE in OCP MX e4m3, decode and encode, Wan2.2 and Wan2.1.

Yardstick: oracle.vae with causal_conv patched inside this file — for every `*.residual.2` / `*.residual.6` 3x3x3 convolution whose input
width is a multiple of 128 the bf16-rounded input is fake-quantised in MX blocks of 32 channels (tests/conv_f8_cases.py: mx_quantise, the
device's exponent rule) and the bf16-rounded weights per output channel (amax / 448). Nothing under oracle/ is edited.

  (a) rel-L2(device fp8, fake-quant oracle) <= rel-L2(device bf16, plain oracle) + E_q, E_q = rel-L2(fake-quant oracle, plain oracle), computed
      here and printed (the issue's CPU figures, for orientation: 6.5e-2 (2.2) / 4.7e-2 (2.1) for decode); 0 < E_q < 0.2.
  (b) option off -> bit-identical to an engine that never had the option; off -> on -> off -> on repeats bit for bit.
  (c) engine.group = 1 and 8 give bit-identical outputs with the option on.
  (d) the engine has no two-call decode with a shared cache: the chunked walk inside one call (3 latent frames, group = 1: one latent frame per
      pass, the oracle's own walk) is the one held to (a).
  (e) all outputs finite.
At least one convolution of each of decode and encode must have taken the f8 route (calls of V.conv3d_cl_f8mx and of the patched oracle
branch are counted): otherwise the comparison shows nothing. Fails without the feature: the attribute and the exports do not exist."""
import sys

import pytest
import torch

import conv_f8_cases as cc
from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

from oracle import vae as ovae  # noqa: E402
from yume_amd import synth  # noqa: E402
from yume_amd import vae_ops as V  # noqa: E402

DEV = "cuda"
CONFIGS = {"2.2": dict(dim=32, dec_dim=128), "2.1": dict(dim=32)}


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def build_vae(cfg, seed):
    if cfg["version"] == "2.2":
        from yume_amd.wan23.modules.vae2_2 import Wan2_2_VAE, WanVAE_
        m = WanVAE_(dim=cfg["dim"], dec_dim=cfg["dec_dim"], z_dim=cfg["z_dim"], temperal_downsample=cfg["temperal_downsample"])
        wrap = Wan2_2_VAE
    else:
        from yume_amd.wan.modules.vae import WanVAE, WanVAE_
        m = WanVAE_(dim=cfg["dim"], z_dim=cfg["z_dim"], temperal_downsample=cfg["temperal_downsample"])
        wrap = WanVAE
    m.load_state_dict(synth.make_vae_state_dict(cfg, seed), strict=True)
    return wrap(z_dim=cfg["z_dim"], device=DEV, model=m)


def qualifies(name, w):
    return name.endswith((".residual.2", ".residual.6")) and w.shape[1] % 128 == 0 and tuple(w.shape[2:]) == (3, 3, 3)


def fake_quant_oracle(monkeypatch, counter):
    """oracle.vae.causal_conv with the qualifying convolutions fake-quantised (module docstring)"""
    plain = ovae.causal_conv
    wcache = {}

    def conv(sd, name, x, cache):
        w = sd[name + ".weight"]
        if not qualifies(name, w):
            return plain(sd, name, x, cache)
        counter[0] += 1
        C, T, H, W = x.shape
        rows = x.bfloat16().float().permute(1, 2, 3, 0).reshape(-1, C)
        xq = cc.mx_dequantise(*cc.mx_quantise(rows)).view(T, H, W, C).permute(3, 0, 1, 2)
        if name not in wcache:
            wb = w.bfloat16().float()
            s = wb.abs().amax(dim=(1, 2, 3, 4), keepdim=True) / 448.0
            s = torch.where(s > 0, s, torch.ones_like(s))
            wcache[name] = (wb / s).clamp(-448, 448).to(torch.float8_e4m3fn).float() * s
        return plain({name + ".weight": wcache[name], name + ".bias": sd[name + ".bias"]}, name, xq, cache)

    monkeypatch.setattr(ovae, "causal_conv", conv)


@pytest.fixture(scope="module", params=["2.2", "2.1"])
def setup(request):
    version = request.param
    cfg = synth.tiny_vae_cfg(version, **CONFIGS[version])
    sd = synth.make_vae_state_dict(cfg, seed=1)
    g = torch.Generator().manual_seed(19)
    s = 16 if version == "2.2" else 8
    z = torch.randn(cfg["z_dim"], 3, 2, 4, generator=g)
    video = torch.rand(3, 5, 2 * s, 4 * s, generator=g) * 2 - 1
    mp = pytest.MonkeyPatch()
    mp.delenv("YUME_VAE_FP8", raising=False)
    plain = {"dec": ovae.decode(sd, cfg, z), "enc": ovae.encode(sd, cfg, video)}
    n_or = [0]
    fake_quant_oracle(mp, n_or)
    n0 = n_or[0]
    fq = {"dec": ovae.decode(sd, cfg, z)}
    n_dec = n_or[0] - n0
    fq["enc"] = ovae.encode(sd, cfg, video)
    n_enc = n_or[0] - n0 - n_dec
    mp.undo()
    mp.delenv("YUME_VAE_FP8", raising=False)
    never = build_vae(cfg, 1)                                       # an engine that never has the option switched
    assert never.model.engine.fp8_conv is False
    vae = build_vae(cfg, 1)
    yield dict(version=version, cfg=cfg, z=z.to(DEV), video=video.to(DEV), plain=plain, fq=fq, n_or=(n_dec, n_enc), never=never, vae=vae)
    mp.undo()


def run(vae, st, what):
    return (vae.decode([st["z"]])[0] if what == "dec" else vae.encode([st["video"]])[0]).cpu()


@pytest.mark.parametrize("what", ["dec", "enc"])
def test_fp8_conv_against_the_fake_quant_oracle_and_off_is_untouched(setup, what, monkeypatch):
    st = setup
    vae, eng = st["vae"], st["vae"].model.engine
    calls = [0]
    real = V.conv3d_cl_f8mx

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(V, "conv3d_cl_f8mx", counted)
    base = run(st["never"], st, what)
    outs = []
    for on in (False, True, False, True):
        eng.fp8_conv = on
        before = calls[0]
        outs.append(run(vae, st, what))
        assert (calls[0] > before) == on                            # the f8 route is taken with the option on, and only then
    eng.fp8_conv = False
    off1, on1, off2, on2 = outs
    # (b)
    assert torch.equal(off1, base) and torch.equal(off2, base)
    assert torch.equal(on1, on2) and not torch.equal(on1, base)
    # the comparison is about something: both sides ran quantised convolutions
    n_or = st["n_or"][0 if what == "dec" else 1]
    assert n_or > 0 and calls[0] > 0
    # (e)
    assert torch.isfinite(on1).all() and on1.shape == st["plain"][what].shape
    # (a) / (d)
    plain, fq = st["plain"][what], st["fq"][what]
    e_q = rel_l2(fq, plain)
    e_bf16 = rel_l2(base, plain)
    e_fp8 = rel_l2(on1, fq)
    print(f"vae {st['version']} {what}: E_q {e_q:.3e}; device bf16 vs plain oracle {e_bf16:.3e}; device fp8 vs fake-quant oracle {e_fp8:.3e}; "
          f"device fp8 vs plain oracle {rel_l2(on1, plain):.3e}; f8 convolutions: oracle {n_or}, device calls {calls[0]}")
    assert 0 < e_q < 0.2
    assert e_fp8 <= e_bf16 + e_q


@pytest.mark.parametrize("what", ["dec", "enc"])
def test_grouped_passes_equal_the_one_chunk_walk_bit_for_bit_with_the_option_on(setup, what):
    st = setup
    vae, eng = st["vae"], st["vae"].model.engine
    keep = eng.group
    eng.fp8_conv = True
    try:
        outs = []
        for group in (1, 8):
            eng.group = group
            outs.append(run(vae, st, what))
    finally:
        eng.group = keep
        eng.fp8_conv = False
    # (c); with group = 1 the device walks the oracle's own chunks, so (a) held on the default group holds on this walk too (d)
    assert torch.equal(outs[0], outs[1])
    e_q, e_bf16 = rel_l2(st["fq"][what], st["plain"][what]), rel_l2(run(st["never"], st, what), st["plain"][what])
    assert rel_l2(outs[0], st["fq"][what]) <= e_bf16 + e_q


def test_env_switch_is_read_when_the_engine_is_built_and_the_pack_holds_the_bytes(setup, monkeypatch):
    st = setup
    monkeypatch.setenv("YUME_VAE_FP8", "1")
    vae = build_vae(st["cfg"], 1)
    eng = vae.model.engine
    assert eng.fp8_conv is True
    eng.ensure_packed()
    n = 0
    for name, p in eng.P.items():
        if isinstance(p, dict):
            q = name.endswith((".residual.2", ".residual.6")) and p["ci"] % 128 == 0 and p["k"] == (3, 3, 3)
            assert ("wq" in p) == q, name
            if q:
                n += 1
                assert p["wq"].dtype == torch.uint8 and tuple(p["wq"].shape) == (p["cop"], 27 * p["ci"]) and tuple(p["sw"].shape) == (p["cop"],)
                amax = p["w"].float().abs().amax(dim=1)
                assert torch.allclose(p["sw"], torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)), rtol=1e-6, atol=0)
    assert n > 0
    eng.fp8_conv = False
    eng.ensure_packed()                                             # part of the pack key: off repacks without the bytes
    assert not any("wq" in p for p in eng.P.values() if isinstance(p, dict))
