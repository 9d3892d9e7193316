"""VaeEngine.fold_upsample (r21): the decoder's nearest-2x + Conv2d 3x3 as four 2x2 phase convolutions, Wan2.2 and Wan2.1.

Yardstick: oracle.vae with `resample` patched inside this file — for every upsample Resample whose 3x3 convolution upfold_qualifies names, the
four phase convolutions run in the oracle's precision on fold_upsample_weight's bytes (the bf16-rounded weight folded and rounded once
more, exactly what the engine packs). Nothing under oracle/ is edited. Tiny configs: 2.2 at dim=32, dec_dim=128 (512 / 512 / 256 all fold),
2.1 at dim=96 (384 -> 192 folds twice, 192 -> 96 does not); z = randn(z_dim, 3, 2, 4).

  (a) rel-L2(device fold, fold oracle) <= rel-L2(device off, plain oracle) + E_f, E_f = rel-L2(fold oracle, plain oracle), computed here and
      printed; 0 < E_f < 1e-2 (a cap, about twice what the fold alone gives on the CPU at these configs: 3.2e-3 and 4.7e-3).
  (b) option off -> bit-identical to an engine that never had the option; off -> on -> off -> on repeats bit for bit; on differs from off.
  (c) engine.group = 1 and 8 give bit-identical outputs with the option on.
  (d) the chunked walk inside one call (3 latent frames, group = 1: one latent frame per pass, the oracle's own walk) is held to (a).
  (e) with fp8_conv also on, (a) in the same form with both patches installed in the oracle (the fake-quant patch of
      tests/test_vae_fp8_gpu.py restated here); the encode output is bit-identical to the option off.
Device calls of V.conv_up2_fold and oracle calls of the patched branch are counted: both > 0 for decode and 0 for encode.
Fails without the feature: the attribute, the two pure functions and the export do not exist."""
import sys

import pytest
import torch
import torch.nn.functional as F

import conv_f8_cases as cc
from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

from oracle import vae as ovae  # noqa: E402
from yume_amd import synth  # noqa: E402
from yume_amd import vae as yvae  # noqa: E402
from yume_amd import vae_ops as V  # noqa: E402

DEV = "cuda"
CONFIGS = {"2.2": dict(dim=32, dec_dim=128), "2.1": dict(dim=96)}
FOLDS = {"2.2": [(512, 512), (512, 512), (256, 256)], "2.1": [(384, 192), (384, 192)]}     # (cin, cout) of the convolutions that fold


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


def fold_oracle(monkeypatch, counter):
    """oracle.vae.resample with the qualifying upsample convolutions run as four phase convolutions on the folded bytes"""
    plain = ovae.resample
    wcache = {}

    def resample(sd, name, x, mode, cache, first_chunk):
        w = sd[name + ".resample.1.weight"]
        if not mode.startswith("upsample") or not yvae.upfold_qualifies(w.shape[1], w.shape[0]):
            return plain(sd, name, x, mode, cache, first_chunk)
        counter[0] += 1
        C, T, H, W = x.shape
        if mode == "upsample3d" and not first_chunk:                      # the time_conv in front: oracle.vae.resample's own lines
            tc = name + ".time_conv"
            y = ovae.causal_conv(sd, tc, x, cache)
            if cache.d[tc].shape[1] < 2:
                cache.d[tc] = torch.cat([torch.zeros_like(cache.d[tc]), cache.d[tc]], dim=1)
            y = y.reshape(2, C, T, H, W)
            x = torch.stack((y[0], y[1]), dim=2).reshape(C, 2 * T, H, W)
        if name not in wcache:
            wcache[name] = yvae.fold_upsample_weight(w.bfloat16()).to(x.dtype).permute(0, 1, 4, 2, 3).contiguous()     # [4, co, ci, 2, 2]
        wf, b = wcache[name], sd[name + ".resample.1.bias"]
        xf = x.permute(1, 0, 2, 3)                                         # [T, C, H, W]
        out = xf.new_zeros(xf.shape[0], w.shape[0], 2 * H, 2 * W)
        for eh in range(2):
            for ew in range(2):
                # tap (th, tw) of output (2a + e_h, 2b + e_w) reads input (a + th - (1 - e_h), b + tw - (1 - e_w)), zero outside
                out[:, :, eh::2, ew::2] = F.conv2d(F.pad(xf, (1 - ew, ew, 1 - eh, eh)), wf[2 * eh + ew], b)
        return out.permute(1, 0, 2, 3)

    monkeypatch.setattr(ovae, "resample", resample)


def fp8_qualifies(name, w):
    return name.endswith((".residual.2", ".residual.6")) and w.shape[1] % 128 == 0 and tuple(w.shape[2:]) == (3, 3, 3)


def fake_quant_oracle(monkeypatch):
    """oracle.vae.causal_conv with the convolutions fp8_conv takes fake-quantised: the bf16-rounded input in MX blocks of 32 channels
    (tests/conv_f8_cases.py), the bf16-rounded weights per output channel (amax / 448) — tests/test_vae_fp8_gpu.py's recipe"""
    plain = ovae.causal_conv
    wcache = {}

    def conv(sd, name, x, cache):
        w = sd[name + ".weight"]
        if not fp8_qualifies(name, w):
            return plain(sd, name, x, cache)
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
    g = torch.Generator().manual_seed(20)
    s = 16 if version == "2.2" else 8
    z = torch.randn(cfg["z_dim"], 3, 2, 4, generator=g)
    video = torch.rand(3, 5, 2 * s, 4 * s, generator=g) * 2 - 1
    mp = pytest.MonkeyPatch()
    mp.delenv("YUME_VAE_UPFOLD", raising=False)
    mp.delenv("YUME_VAE_FP8", raising=False)
    plain = ovae.decode(sd, cfg, z)
    n_or = [0]
    fold_oracle(mp, n_or)
    fold = ovae.decode(sd, cfg, z)
    n_dec = n_or[0]
    ovae.encode(sd, cfg, video)
    n_enc = n_or[0] - n_dec
    fake_quant_oracle(mp)
    both = ovae.decode(sd, cfg, z)
    mp.undo()
    mp.delenv("YUME_VAE_UPFOLD", raising=False)
    mp.delenv("YUME_VAE_FP8", raising=False)
    never = build_vae(cfg, 1)                                       # an engine that never has the option switched
    assert never.model.engine.fold_upsample is False and never.model.engine.fp8_conv is False
    vae = build_vae(cfg, 1)
    yield dict(version=version, cfg=cfg, z=z.to(DEV), video=video.to(DEV), plain=plain, fold=fold, both=both, n_or=(n_dec, n_enc), never=never, vae=vae)
    mp.undo()


def run(vae, st, what):
    return (vae.decode([st["z"]])[0] if what == "dec" else vae.encode([st["video"]])[0]).cpu()


@pytest.fixture()
def calls(monkeypatch):
    n = [0]
    real = V.conv_up2_fold

    def counted(*a, **k):
        n[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(V, "conv_up2_fold", counted)
    return n


def test_fold_against_the_fold_oracle_and_off_is_untouched(setup, calls):
    st = setup
    vae, eng = st["vae"], st["vae"].model.engine
    base = run(st["never"], st, "dec")
    outs = []
    for on in (False, True, False, True):
        eng.fold_upsample = on
        before = calls[0]
        outs.append(run(vae, st, "dec"))
        assert (calls[0] > before) == on                            # the folded route is taken with the option on, and only then
    eng.fold_upsample = False
    off1, on1, off2, on2 = outs
    # (b)
    assert torch.equal(off1, base) and torch.equal(off2, base)
    assert torch.equal(on1, on2) and not torch.equal(on1, base)
    # the comparison is about something: both sides ran folded convolutions — the oracle once per latent frame, the device once per pass
    assert st["n_or"][0] == 3 * len(FOLDS[st["version"]]) > 0
    assert calls[0] == 2 * len(yvae.decode_passes(3, eng.group)) * len(FOLDS[st["version"]]) > 0
    assert torch.isfinite(on1).all() and on1.shape == st["plain"].shape
    # (a)
    e_f = rel_l2(st["fold"], st["plain"])
    e_off = rel_l2(base, st["plain"])
    e_on = rel_l2(on1, st["fold"])
    print(f"vae {st['version']} dec: E_f {e_f:.3e}; device off vs plain oracle {e_off:.3e}; device fold vs fold oracle {e_on:.3e}; "
          f"device fold vs plain oracle {rel_l2(on1, st['plain']):.3e}; folded convolutions: oracle {st['n_or'][0]}, device calls {calls[0]}")
    assert 0 < e_f < 1e-2
    assert e_on <= e_off + e_f


def test_the_pack_holds_the_folded_bytes_for_the_layers_the_rule_names(setup):
    st = setup
    eng = st["vae"].model.engine
    eng.fold_upsample = True
    try:
        eng.ensure_packed()
        got = []
        for name, p in eng.P.items():
            if isinstance(p, dict) and "wf" in p:
                assert name.startswith("decoder.") and name.endswith(".resample.1") and yvae.upfold_qualifies(p["ci"], p["co"]), name
                assert p["wf"].dtype == torch.bfloat16 and tuple(p["wf"].shape) == (4, p["cop"], 4 * p["ci"])
                w3 = p["w"][:p["co"], :9 * p["ci"]].reshape(p["co"], 3, 3, p["ci"]).permute(0, 3, 1, 2)     # the packed bf16 bytes
                assert torch.equal(p["wf"][:, :p["co"]], yvae.fold_upsample_weight(w3).reshape(4, p["co"], 4 * p["ci"]))
                got.append((p["ci"], p["co"]))
        assert sorted(got) == sorted(FOLDS[st["version"]])
        ups = [p for n, p in eng.P.items() if isinstance(p, dict) and n.startswith("decoder.") and n.endswith(".resample.1")]
        assert len(ups) == 3 and not any("wf" in p for n, p in eng.P.items() if isinstance(p, dict) and n.startswith("encoder."))
    finally:
        eng.fold_upsample = False
    eng.ensure_packed()                                             # part of the pack key: off repacks without the bytes
    assert not any("wf" in p for p in eng.P.values() if isinstance(p, dict))


def test_grouped_passes_equal_the_one_latent_walk_bit_for_bit_with_the_option_on(setup, calls):
    st = setup
    vae, eng = st["vae"], st["vae"].model.engine
    keep = eng.group
    eng.fold_upsample = True
    try:
        outs = []
        for group in (1, 8):
            eng.group = group
            outs.append(run(vae, st, "dec"))
    finally:
        eng.group = keep
        eng.fold_upsample = False
    # (c); with group = 1 the device walks the oracle's own chunks: (d)
    assert torch.equal(outs[0], outs[1])
    assert calls[0] == (3 + 2) * len(FOLDS[st["version"]])
    e_f, e_off = rel_l2(st["fold"], st["plain"]), rel_l2(run(st["never"], st, "dec"), st["plain"])
    e_on = rel_l2(outs[0], st["fold"])
    print(f"vae {st['version']} dec, group = 1: device fold vs fold oracle {e_on:.3e} <= {e_off:.3e} + {e_f:.3e}")
    assert e_on <= e_off + e_f


def test_with_fp8_conv_also_on_and_the_encoder_is_untouched(setup, calls):
    st = setup
    vae, eng = st["vae"], st["vae"].model.engine
    enc_off = run(st["never"], st, "enc")
    base = run(st["never"], st, "dec")
    eng.fold_upsample = True
    try:
        enc_on = run(vae, st, "enc")
        assert calls[0] == 0 and st["n_or"][1] == 0                 # no folded convolution in the encoder, on the device or in the oracle
        assert torch.equal(enc_on, enc_off)
        eng.fp8_conv = True
        on = run(vae, st, "dec")
        assert calls[0] > 0
    finally:
        eng.fold_upsample = False
        eng.fp8_conv = False
    # (e)
    e_both = rel_l2(st["both"], st["plain"])
    e_off = rel_l2(base, st["plain"])
    e_on = rel_l2(on, st["both"])
    print(f"vae {st['version']} dec, fold + fp8: E {e_both:.3e}; device off vs plain oracle {e_off:.3e}; device both vs both-patched oracle {e_on:.3e}")
    assert torch.isfinite(on).all()
    assert 0 < e_both < 0.2 + 1e-2                                  # the two caps of the two options' own tests
    assert e_on <= e_off + e_both
    assert torch.equal(run(vae, st, "dec"), base)                   # both options off again: the parent's bits


def test_env_switch_is_read_when_the_engine_is_built(setup, monkeypatch):
    monkeypatch.setenv("YUME_VAE_UPFOLD", "1")
    eng = build_vae(setup["cfg"], 1).model.engine
    assert eng.fold_upsample is True and eng.fp8_conv is False
