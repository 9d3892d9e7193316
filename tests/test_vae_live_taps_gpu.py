"""VaeEngine.live_taps (r24) at engine level, Wan2.2 and Wan2.1, decode and encode: the first pass (one frame, an empty cache) runs its
causal 3x3x3 convolutions on the nine taps of dt = 2 alone. The same value in real arithmetic: no tolerance of this file's own.

  1. V.conv3d_cl / V.conv3d_cl_f8mx wrapped to record (pass, k, stride, pad, T, has_cache, multiplies): option on -> no call of the first pass
     has k[0] == 3 and every other record equals the off leg's; off -> the record of an engine that never had the option; the multiply
     count drops by exactly 18/27 of the first pass's 3x3x3 calls, one per 3x3x3 weight of the coder.
  2. against the committed fixtures (vae_22, vae_21: the reference's outputs; live_vae: further outputs of the reference) the on leg meets
     the tolerance of tests/test_vae_gpu.py (rel-L2 <= 3e-2) and E_on <= 1.5 E_off — the margin tests/test_forward_batch_gpu.py gives a path
     that is equal in real arithmetic. E_on / E_off is printed.
  3. group = 1 and group = 8 agree bit for bit with the option on.
  4. off -> on -> off -> on returns the same bits per setting; off equals an engine that never had the option.
  5. a one-latent decode and a one-frame encode (nothing but a first pass) meet the tolerance of item 2 against the oracle.
  6. with fp8_conv and / or fold_upsample also on: the bounds of tests/test_vae_fp8_gpu.py / tests/test_vae_upfold_gpu.py, against the
     oracle patched as those files patch it (their helpers are imported, their tiny configs used).
Fails without the feature: the attribute does not exist and the first pass keeps its 27-tap calls."""
import sys

import pytest
import torch

from conftest import ROOT, load_golden
import test_vae_upfold_gpu as up

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

from oracle import vae as ovae  # noqa: E402
from yume_amd import synth  # noqa: E402
from yume_amd import vae as yvae  # noqa: E402
from yume_amd import vae_ops as V  # noqa: E402

DEV = "cuda"
TOL = 3e-2                      # tests/test_vae_gpu.py: rel-L2 on decoded pixels and on encoded latents
MARGIN = 1.5                    # tests/test_forward_batch_gpu.py: a path equal in real arithmetic


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    for v in ("YUME_VAE_LIVE_TAPS", "YUME_VAE_FP8", "YUME_VAE_UPFOLD", "YUME_VAE_GROUP"):
        monkeypatch.delenv(v, raising=False)


_FX = {}


def fixture(name):
    """{cfg, seed, z, video, dec, enc (the reference's), never, vae}: one pair of engines per fixture, shared by the tests"""
    if name not in _FX:
        fx = load_golden(name)
        d = dict(cfg=fx["cfg"], seed=fx["seed"], z=fx["z"].to(DEV), video=fx["video"].to(DEV), dec=fx["dec"], enc=fx["enc"])
        d["never"], d["vae"] = up.build_vae(d["cfg"], d["seed"]), up.build_vae(d["cfg"], d["seed"])
        assert d["never"].model.engine.live_taps is False
        _FX[name] = d
    return _FX[name]


def run(vae, st, what):
    return (vae.decode([st["z"]])[0] if what == "dec" else vae.encode([st["video"]])[0]).cpu()


class Recorder:
    """wraps the two convolution wrappers of yume_amd.vae_ops and the engine's pass functions"""

    def __init__(self, monkeypatch, eng):
        self.rec, self.npass = [], 0
        real, real8 = V.conv3d_cl, V.conv3d_cl_f8mx
        rec = self

        def conv(x, cache, w, bias, cout, k, stride, pad, ups, out, epi=V.EPI_BF16, **kw):
            to = out.shape[0] // 2 if epi == V.EPI_TSPLIT else out.shape[0]
            mult = to * out.shape[1] * out.shape[2] * cout * x.shape[3] * k[0] * k[1] * k[2]
            rec.rec.append((rec.npass, "bf16", tuple(k), tuple(stride), tuple(pad), x.shape[0], cache is not None, mult))
            return real(x, cache, w, bias, cout, k, stride, pad, ups, out, epi, **kw)

        def conv8(xq, xe, cache, wq, sw, bias, cout, k, out, *a, **kw):
            mult = out.shape[0] * out.shape[1] * out.shape[2] * cout * xq.shape[3] * k[0] * k[1] * k[2]
            rec.rec.append((rec.npass, "f8", tuple(k), (1, 1, 1), (k[0] - 1, k[1] // 2, k[2] // 2), xq.shape[0], cache is not None, mult))
            return real8(xq, xe, cache, wq, sw, bias, cout, k, out, *a, **kw)

        monkeypatch.setattr(V, "conv3d_cl", conv)
        monkeypatch.setattr(V, "conv3d_cl_f8mx", conv8)
        for fn in ("_decoder_pass", "_encoder_pass"):
            def counted(x, cache, first, _real=getattr(eng, fn)):
                rec.npass += 1
                assert first == (rec.npass == 1)
                return _real(x, cache, first)
            monkeypatch.setattr(eng, fn, counted)

    def take(self):
        r, self.rec, self.npass = self.rec, [], 0
        return r


def _is_dead_tap_call(r):
    """the rule, restated: a causal 3-tap convolution of stride 1 over one frame with no cache"""
    _, _, k, stride, pad, T, has_cache, _ = r
    return k[0] == 3 and pad[0] == 2 and stride == (1, 1, 1) and T == 1 and not has_cache


def _one_frame(r):
    p, kind, k, stride, pad, T, hc, mult = r
    return (p, kind, (1, k[1], k[2]), stride, (0, pad[1], pad[2]), T, hc, mult // 3)


@pytest.mark.parametrize("what", ["dec", "enc"])
@pytest.mark.parametrize("name", ["vae_22", "vae_21"])
def test_first_pass_runs_no_three_tap_call_and_every_other_record_is_unchanged(name, what):
    st = fixture(name)
    with pytest.MonkeyPatch.context() as mp:
        never_rec = Recorder(mp, st["never"].model.engine)
        run(st["never"], st, what)
        parent = never_rec.take()
    eng = st["vae"].model.engine
    with pytest.MonkeyPatch.context() as mp:
        rec = Recorder(mp, eng)
        try:
            run(st["vae"], st, what)
            off = rec.take()
            eng.live_taps = True
            run(st["vae"], st, what)
            on = rec.take()
        finally:
            eng.live_taps = False
    assert off == parent                                                    # option off: the parent's calls
    dead = [r for r in off if _is_dead_tap_call(r)]
    coder = "decoder." if what == "dec" else "encoder."
    n333 = sum(1 for k, v in synth.make_vae_state_dict(st["cfg"], st["seed"]).items()
               if k.startswith(coder) and k.endswith(".weight") and tuple(v.shape[2:]) == (3, 3, 3))
    assert len(dead) == n333 > 0 and all(r[0] == 1 for r in dead)           # every 3x3x3 convolution of the coder, once, in the first pass
    assert max(r[0] for r in off) >= 2                                      # the fixture has later passes, which must stay as they are
    assert not any(r[2][0] == 3 for r in on if r[0] == 1)
    assert on == [_one_frame(r) if _is_dead_tap_call(r) else r for r in off]
    saved = sum(r[-1] for r in off) - sum(r[-1] for r in on)
    assert saved == sum(r[-1] // 27 * 18 for r in dead) > 0
    print(f"{name} {what}: {len(dead)} first-pass 3x3x3 calls, multiplies {sum(r[-1] for r in off):.4g} -> {sum(r[-1] for r in on):.4g}")


@pytest.mark.parametrize("what", ["dec", "enc"])
@pytest.mark.parametrize("name", ["vae_22", "vae_21"])
def test_on_leg_meets_the_fixture_tolerance_toggles_repeat_their_bits_and_groups_agree(name, what):
    st = fixture(name)
    vae, eng = st["vae"], st["vae"].model.engine
    base = run(st["never"], st, what)
    keep = eng.group
    try:
        outs = []
        for on in (False, True, False, True):
            eng.live_taps = on
            outs.append(run(vae, st, what))
        groups = []
        for group in (1, 8):
            eng.group = group
            groups.append(run(vae, st, what))
    finally:
        eng.group = keep
        eng.live_taps = False
    off1, on1, off2, on2 = outs
    assert torch.equal(off1, base) and torch.equal(off2, base)              # 4.
    assert torch.equal(on1, on2)
    assert torch.equal(groups[0], groups[1])                                # 3.
    e_off, e_on = rel_l2(base, st[what]), rel_l2(on1, st[what])             # 2.
    print(f"{name} {what}: E_off {e_off:.6e} E_on {e_on:.6e} E_on / E_off {e_on / e_off:.6f} on == off bits: {torch.equal(on1, base)}")
    assert torch.isfinite(on1).all() and on1.shape == st[what].shape
    assert e_on <= TOL
    assert e_on <= MARGIN * e_off


def _live_err_rel(got, want):
    """rel-L2 of `got` against an output stored by oracle/make_golden_live.py (whole, or its seeded sample of elements)"""
    got = got.detach().cpu()
    if "full" in want:
        assert got.shape == want["full"].shape
        return rel_l2(got, want["full"])
    assert tuple(got.shape) == tuple(want["shape"])
    return rel_l2(got.reshape(-1)[want["idx"].long()], want["values"])


@pytest.mark.parametrize("ver,T", [("2.2", 1), ("2.2", 5), ("2.1", 2), ("2.1", 4)])
def test_live_vae_fixture_on_leg_meets_the_tolerance(ver, T):
    """tests/golden/live_vae.pt (the inputs of tests/test_oracle_vae.py): 16-channel levels — the copy branch of the weights — and, at
    ("2.2", 1), a one-latent decode and a 3-frame (one chunk) encode: nothing but a first pass"""
    cfg = synth.tiny_vae_cfg(ver, dim=16)
    if ver == "2.2":
        cfg["dec_dim"] = 16
    want = load_golden("live_vae")[(ver, T)]
    g = torch.Generator().manual_seed(T)
    z = torch.randn(cfg["z_dim"], T, 2, 4, generator=g)
    s = 16 if ver == "2.2" else 8
    video = torch.rand(3, 1 + 4 * (T - 1) + 2, 2 * s, 4 * s, generator=g) * 2 - 1
    vae = up.build_vae(cfg, 31)
    eng = vae.model.engine
    res = {}
    for on in (False, True):
        eng.live_taps = on
        res[on] = (vae.decode([z.to(DEV)])[0].cpu(), vae.encode([video.to(DEV)])[0].cpu())
    eng.ensure_packed()
    assert any("wl" in p for p in eng.P.values() if isinstance(p, dict))    # the copy branch ran
    for i, what in enumerate(("dec", "enc")):
        e_off, e_on = _live_err_rel(res[False][i], want[what]), _live_err_rel(res[True][i], want[what])
        print(f"live_vae {ver} T={T} {what}: E_off {e_off:.6e} E_on {e_on:.6e} E_on / E_off {e_on / e_off:.6f}")
        assert torch.isfinite(res[True][i]).all()
        assert e_on <= TOL
        assert e_on <= MARGIN * e_off


@pytest.mark.parametrize("name", ["vae_22", "vae_21"])
def test_one_latent_decode_and_one_frame_encode(name):
    st = fixture(name)
    sd = synth.make_vae_state_dict(st["cfg"], st["seed"])
    z1, v1 = st["z"][:, :1], st["video"][:, :1]
    want = (ovae.decode(sd, st["cfg"], z1.cpu()), ovae.encode(sd, st["cfg"], v1.cpu()))
    vae, eng = st["vae"], st["vae"].model.engine
    res = {}
    try:
        for on in (False, True):
            eng.live_taps = on
            res[on] = (vae.decode([z1])[0].cpu(), vae.encode([v1])[0].cpu())
    finally:
        eng.live_taps = False
    for i, what in enumerate(("dec", "enc")):
        e_off, e_on = rel_l2(res[False][i], want[i]), rel_l2(res[True][i], want[i])
        print(f"{name} one-frame {what}: E_off {e_off:.6e} E_on {e_on:.6e} E_on / E_off {e_on / e_off:.6f}")
        assert res[True][i].shape == want[i].shape and torch.isfinite(res[True][i]).all()
        assert e_on <= TOL
        assert e_on <= MARGIN * e_off


def test_the_pack_holds_a_copy_only_where_the_view_does_not_fit_and_the_key_holds_the_option():
    st = fixture("vae_22")
    eng = st["vae"].model.engine
    eng.live_taps = True
    try:
        eng.ensure_packed()
        n = 0
        for name, p in eng.P.items():
            if not isinstance(p, dict):
                continue
            want = p["k"][0] == 3 and not yvae.live_view_fits(p["k"], p["cip"])
            assert ("wl" in p) == want, name
            if want:
                n += 1
                kl = p["k"][1] * p["k"][2] * p["cip"]
                assert tuple(p["wl"].shape) == (p["cop"], (kl + 63) // 64 * 64) and p["wl"].dtype == torch.bfloat16
                assert torch.equal(p["wl"][:, :kl], p["w"][:, 2 * kl:3 * kl]) and not p["wl"][:, kl:].any()
        assert n > 0                                                        # encoder.conv1: 12 (16) input channels
    finally:
        eng.live_taps = False
    eng.ensure_packed()
    assert not any("wl" in p for p in eng.P.values() if isinstance(p, dict))


def test_env_switch_is_read_when_the_engine_is_built(monkeypatch):
    st = fixture("vae_21")
    monkeypatch.setenv("YUME_VAE_LIVE_TAPS", "1")
    eng = up.build_vae(st["cfg"], st["seed"]).model.engine
    assert eng.live_taps is True and eng.fp8_conv is False and eng.fold_upsample is False


# ------------------------------------------------------------------------------------------------ 6. with the other two options
@pytest.fixture(scope="module", params=["2.2", "2.1"])
def combo(request):
    """the tiny configs and the patched oracles of tests/test_vae_upfold_gpu.py; oracle outputs once per version"""
    version = request.param
    cfg = synth.tiny_vae_cfg(version, **up.CONFIGS[version])
    sd = synth.make_vae_state_dict(cfg, seed=1)
    g = torch.Generator().manual_seed(20)
    s = 16 if version == "2.2" else 8
    z = torch.randn(cfg["z_dim"], 3, 2, 4, generator=g)
    video = torch.rand(3, 5, 2 * s, 4 * s, generator=g) * 2 - 1
    mp = pytest.MonkeyPatch()
    for v in ("YUME_VAE_LIVE_TAPS", "YUME_VAE_FP8", "YUME_VAE_UPFOLD", "YUME_VAE_GROUP"):
        mp.delenv(v, raising=False)
    orc = {(False, False): (ovae.decode(sd, cfg, z), ovae.encode(sd, cfg, video))}
    up.fold_oracle(mp, [0])
    orc[(False, True)] = (ovae.decode(sd, cfg, z), orc[(False, False)][1])              # the fold does not touch the encoder
    up.fake_quant_oracle(mp)
    orc[(True, True)] = (ovae.decode(sd, cfg, z), ovae.encode(sd, cfg, video))
    mp.undo()
    up.fake_quant_oracle(mp)
    orc[(True, False)] = (ovae.decode(sd, cfg, z), orc[(True, True)][1])
    mp.undo()
    vae = up.build_vae(cfg, 1)
    base = (vae.decode([z.to(DEV)])[0].cpu(), vae.encode([video.to(DEV)])[0].cpu())
    return dict(version=version, z=z.to(DEV), video=video.to(DEV), orc=orc, vae=vae, base=base)


@pytest.mark.parametrize("fp8,fold", [(False, False), (False, True), (True, False), (True, True)])
def test_all_four_combinations_with_fp8_conv_and_fold_upsample(combo, fp8, fold):
    st = combo
    vae, eng = st["vae"], st["vae"].model.engine
    plain = st["orc"][(False, False)]
    try:
        eng.fp8_conv, eng.fold_upsample = fp8, fold
        eng.live_taps = False
        off = (vae.decode([st["z"]])[0].cpu(), vae.encode([st["video"]])[0].cpu())
        eng.live_taps = True
        on = (vae.decode([st["z"]])[0].cpu(), vae.encode([st["video"]])[0].cpu())
    finally:
        eng.fp8_conv = eng.fold_upsample = eng.live_taps = False
    for i, what in enumerate(("dec", "enc")):
        patched = st["orc"][(fp8, fold)][i]
        e_opt = rel_l2(patched, plain[i])                   # E_q / E_f / both: what the options themselves cost, in the oracle
        e_base = rel_l2(st["base"][i], plain[i])            # the device with every option off against the plain oracle
        e_off, e_on = rel_l2(off[i], patched), rel_l2(on[i], patched)
        print(f"vae {st['version']} {what} fp8={fp8} fold={fold}: E_opt {e_opt:.3e} device-off-all {e_base:.3e}; live off {e_off:.6e} on {e_on:.6e} "
              f"ratio {e_on / e_off:.6f}")
        assert torch.isfinite(on[i]).all() and on[i].shape == plain[i].shape
        assert e_opt < 0.2 + 1e-2                           # the caps of the two options' own tests
        if fp8 or fold:
            assert e_on <= e_base + e_opt                   # the bound of tests/test_vae_fp8_gpu.py / tests/test_vae_upfold_gpu.py
        else:
            assert e_on <= TOL and e_on <= MARGIN * e_off
