"""TEST INFRASTRUCTURE — golden vectors of the checks that used to execute the REAL reference inside the test run.

Those tests (tests/test_oracle_dit.py, test_oracle_vae.py, test_oracle_t5.py, test_oracle_clip.py, test_attention_seam.py,
test_ulysses_cpu.py, test_sampling.py, test_frames.py, test_boundary_cpu.py) now read what the reference computed on their seeded inputs
from tests/golden/live_*.pt, so the suite runs from the repository alone. This script runs the reference on exactly those inputs (the
cases and seeds below are the tests' own) and writes the fixtures.

    python oracle/make_golden_live.py            # build container only (needs the reference tree, oracle/ref_import.py)

An output larger than FULL_LIMIT elements is stored as SAMPLE elements at sorted indices drawn from a fixed seed, next to its shape and
its fp64 norm; everything else is stored whole.
"""
import os
import socket
import sys
import tempfile
import types

import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_import, ref_scripts  # noqa: E402
from yume_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
FULL_LIMIT = 1 << 14
SAMPLE = 1 << 13

DIT_CASES = [("wan23", 15, 8, True), ("wan23", 32, 8, True), ("wan23", 3, 8, False), ("wan", 16, 9, True), ("wan", 12, 8, True),
             ("wan", 3, 9, False), ("wan23", 40, 8, True), ("wan23", 110, 8, True), ("wan23", 360, 8, True), ("wan", 100, 9, True)]
DIT_NOQK_CASES = [("wan23", 15, 8, True), ("wan23", 3, 8, False), ("wan", 16, 9, True)]
VAE_CASES = [("2.2", 1), ("2.2", 5), ("2.1", 2), ("2.1", 4)]
ATTN_SHAPES = [(1, 33, 47, 2, 128), (2, 64, 64, 3, 80), (1, 5, 300, 1, 64)]
ULYSSES_CASES = [(2, 48, 4), (4, 64, 8)]
CLEAN_TEXTS = ['  a  cat &amp;amp; a\tdog \n\n walk  ', '&lt;b&gt;bold&lt;/b&gt;', '', '  ', 'x', 'café \xa0 au   lait', 'a&nbsp;b', '  A &amp;amp; B\n\n walks   through\tthe cityâ€™s  &lt;gate&gt;  ']     # tests/test_boundary_cpu.py's inputs, byte for byte


def pack(t):
    """a tensor -> {"full": t} or, past FULL_LIMIT elements, a seeded sample of it (tests/conftest.py::live_close reads either)."""
    t = t.detach().cpu()
    if t.numel() <= FULL_LIMIT:
        return {"full": t.clone()}
    idx = torch.randint(0, t.numel(), (SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values.to(torch.int32)
    return {"shape": tuple(t.shape), "idx": idx, "values": t.reshape(-1)[idx.long()].clone(), "norm": float(t.double().norm())}


def dit_cases():
    from make_golden import build_reference, run_reference, token_count
    from yume_amd import framepack
    out = {}
    for family, F, lfz, packed in DIT_CASES:
        cfg = synth.tiny_cfg(family, layers=1)
        sd = synth.make_dit_state_dict(cfg, family, seed=21)
        ref = build_reference(family, cfg, sd)
        inp = synth.make_dit_inputs(cfg, family, F, 10, 12, n_text=9, seed=22)
        if family == "wan" and packed and lfz != 9:
            L = framepack.pack_plan(F, 10, 12, lfz, F - 9).seq_len
        else:
            L = token_count(family, F, 10, 12, lfz, packed)
        t = torch.cat([torch.zeros(5), torch.full((L - 5,), 333.25)]).unsqueeze(0).double() if family == "wan23" and packed else torch.tensor([250.0])
        want, _ = run_reference(ref, family, inp, t, L, lfz, packed)
        out[(family, F, lfz, packed)] = pack(want)
    return out


def dit_extra_cases():
    from make_golden import build_reference, run_reference, token_count
    noqk = {}
    for family, F, lfz, packed in DIT_NOQK_CASES:
        cfg = dict(synth.tiny_cfg(family, layers=2), qk_norm=False)
        sd = synth.make_dit_state_dict(cfg, family, seed=61)
        ref = build_reference(family, cfg, sd)
        inp = synth.make_dit_inputs(cfg, family, F, 10, 12, n_text=9, seed=62)
        L = token_count(family, F, 10, 12, lfz, packed)
        t = torch.cat([torch.zeros(5), torch.full((L - 5,), 333.25)]).unsqueeze(0).double() if family == "wan23" and packed else torch.tensor([250.0])
        want, _ = run_reference(ref, family, inp, t, L, lfz, packed)
        noqk[(family, F, lfz, packed)] = pack(want)
    from make_golden_cache import reference_cache_run
    from test_oracle_dit import _cache_case
    family, cfg, sd, a, b, L, lfz, cache_list = _cache_case()
    r1, rc, r2 = reference_cache_run(cfg, sd, a, b, L, lfz, cache_list)
    cache = {"out_record": pack(r1), "out_replay": pack(r2), "cache_shapes": [tuple(c.shape) for c in rc]}
    return {"forward_no_qk_norm": noqk, "cache": cache}


def vae_cases():
    from make_golden_vae import build_reference_vae
    from oracle import vae as ovae
    out = {}
    for ver, T in VAE_CASES:
        cfg = synth.tiny_vae_cfg(ver, dim=16)
        if ver == "2.2":
            cfg["dec_dim"] = 16
        sd = synth.make_vae_state_dict(cfg, 31)
        ref = build_reference_vae(cfg, sd)
        mean, inv = ovae.latent_scale(ver)
        g = torch.Generator().manual_seed(T)
        z = torch.randn(cfg["z_dim"], T, 2, 4, generator=g)
        s = 16 if ver == "2.2" else 8
        video = torch.rand(3, 1 + 4 * (T - 1) + 2, 2 * s, 4 * s, generator=g) * 2 - 1
        with torch.no_grad():
            wd = ref.decode(z.unsqueeze(0), [mean, inv])[0].clamp(-1, 1)
            we = ref.encode(video.unsqueeze(0), [mean, inv])[0]
        out[(ver, T)] = {"dec": pack(wd), "enc": pack(we)}
    return out


def t5_case():
    cfg = synth.tiny_t5_cfg(dim=128, heads=2, ffn=192, layers=3, vocab=300)
    sd = synth.make_t5_state_dict(cfg, 9)
    mod = ref_import.ref_t5()
    ref = mod.T5Encoder(cfg["vocab"], cfg["dim"], cfg["dim_attn"], cfg["dim_ffn"], cfg["num_heads"], cfg["num_layers"],
                        cfg["num_buckets"], shared_pos=False, dropout=0.0).eval()
    ref.load_state_dict(sd, strict=True)
    ids = torch.randint(1, cfg["vocab"], (2, 150), generator=torch.Generator().manual_seed(1))
    mask = torch.ones(2, 150, dtype=torch.long)
    mask[1, 101:] = 0
    with torch.no_grad():
        want = ref(ids, mask)
    rel = torch.arange(150).unsqueeze(0) - torch.arange(150).unsqueeze(1)
    buckets = ref.blocks[0].pos_embedding._relative_position_bucket(rel)
    assert int(buckets.max()) < 128
    return {"out0": pack(want[0]), "out1_valid": pack(want[1, :101]), "buckets": buckets.to(torch.int8)}


def clip_case():
    cfg = synth.tiny_clip_cfg(dim=160, heads=2, layers=2, image=42)
    sd = synth.make_clip_state_dict(cfg, 2)
    ref = ref_import.ref_clip().VisionTransformer(**cfg).eval()
    ref.load_state_dict(sd, strict=True)
    x = torch.randn(1, 3, 42, 42, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = ref(x, use_31_block=True)
    return {"out31": pack(want)}


def attention_cases():
    import make_golden_attention as mga
    out = {}
    for family in ("wan", "wan23"):
        att = mga.ref_attention_module(family)
        rows = []
        g = torch.Generator().manual_seed(1)
        for (B, Lq, Lk, N, D) in ATTN_SHAPES:
            q, k, v = (torch.randn(B, L, N, D, generator=g) for L in (Lq, Lk, Lk))
            rows.append({"fp32": pack(att.attention(q, k, v, dtype=torch.float32)), "bf16": pack(att.attention(q, k, v).float())})
        out[family] = {"flash_attn_available": bool(att.FLASH_ATTN_2_AVAILABLE or att.FLASH_ATTN_3_AVAILABLE), "cases": rows}
    return out


def _ulysses_worker(rank, world, port, L, H, path):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from test_ulysses_cpu import D, _global
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ref = ref_import.ref_ulysses()
    q, k, v, Lp = _global(L, H, world)
    rows = slice(rank * Lp, (rank + 1) * Lp)
    shard = lambda t: t[rows].float().view(1, Lp, H, D)
    want = ref.distributed_attention(shard(q), shard(k), shard(v), seq_lens=torch.tensor([L])).reshape(Lp, H * D)
    torch.save(want, f"{path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def ulysses_cases():
    out = {}
    for world, L, H in ULYSSES_CASES:
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        path = os.path.join(tempfile.mkdtemp(), "want")
        mp.spawn(_ulysses_worker, args=(world, port, L, H, path), nprocs=world, join=True)
        out[(world, L, H)] = [pack(torch.load(f"{path}.{r}")) for r in range(world)]
    return out


def sampler_cases():
    """the scripts' own loops on tests/test_sampling.py's inputs: results, model-call sequences, noise-draw counts, 5B timestep vectors"""
    from test_sampling import GOLD as SAMPLER_GOLD, _script_inputs
    from oracle import sampler as osamp
    fx = torch.load(SAMPLER_GOLD, weights_only=False)
    out = {}
    for dtype in (torch.float64, torch.float32):
        c, f, mi, noise, lfz = _script_inputs(fx, dtype)
        r = {}
        sig3 = list(osamp.get_sampling_sigmas(50, 3.0))
        for sde in (True, False):
            ref, draws, calls, span = ref_scripts.run_tts(f, noise.clone(), noise, mi, sig3, lfz, sde=sde, seed=fx["seed_noise"])
            r[("tts", sde)] = {"latent": ref.clone(), "calls": list(calls), "n_draws": len(draws)}
        for n in (50, 6):
            sig = list(osamp.get_sampling_sigmas(n, 3.0))
            ref, calls, _ = ref_scripts.run_euler_14b(f, noise.clone(), noise, mi, sig, lfz)
            r[("euler_14b", n)] = {"latent": ref.clone(), "n_calls": len(calls)}
            sig = list(osamp.get_sampling_sigmas(n, 7.0))
            lat0 = torch.cat([mi[:, :-lfz], noise[:, -lfz:]], dim=1)
            seq_len = c["F"] * (c["H"] // 2) * (c["W"] // 2) + 5
            ref, tvecs, calls, _ = ref_scripts.run_euler_5b(f, lat0.clone(), mi, sig, lfz, seq_len)
            r[("euler_5b", n)] = {"latent": ref.clone(), "n_calls": len(calls), "tvecs": torch.cat([t.clone() for t in tvecs])}
        out[str(dtype).split(".")[-1]] = r
    return out


def webapp_case():
    v = ref_scripts.webapp_case()
    return {"frames": torch.from_numpy(ref_scripts.run_webapp_postprocess(v.clone()))}


def clean_cases():
    """basic_clean + whitespace_clean of wan/modules/tokenizers.py with ftfy.fix_text stubbed to the identity and to the one-replacement
    stand-in of tests/test_boundary_cpu.py"""
    path = os.path.join(ref_import.REF_ROOT, "wan", "modules", "tokenizers.py")
    head = open(path).read().split("class HuggingfaceTokenizer")[0].replace("from transformers import AutoTokenizer", "")
    out = {}
    for name, fix in (("identity", lambda t: t), ("mojibake_quote", lambda s: s.replace("â€™", "'"))):
        stub = types.ModuleType("ftfy")
        stub.fix_text = fix
        saved = sys.modules.get("ftfy")
        sys.modules["ftfy"] = stub
        try:
            ns = {}
            exec(compile(head, path, "exec"), ns)
        finally:
            if saved is None:
                del sys.modules["ftfy"]
            else:
                sys.modules["ftfy"] = saved
        out[name] = {t: ns["whitespace_clean"](ns["basic_clean"](t)) for t in CLEAN_TEXTS}
    return out


def main():
    assert ref_import.available() and ref_scripts.available(), "needs the reference tree"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    files = {"live_dit": dit_cases, "live_dit_extra": dit_extra_cases, "live_vae": vae_cases, "live_sampler": sampler_cases,
             "live_misc": lambda: {"t5": t5_case(), "clip": clip_case(), "attention": attention_cases(), "ulysses": ulysses_cases(),
                                   "webapp": webapp_case(), "clean": clean_cases()}}
    for name, fn in files.items():
        p = os.path.join(GOLD, name + ".pt")
        torch.save(fn(), p)
        print(p, os.path.getsize(p))


if __name__ == "__main__":
    main()
