#!/usr/bin/env python3
"""Reference K/V attended in place (`ops.attention_bnhd_segments`, `kv_dtype=`): rate and memory against the parent commit.

Two measurements, each in child processes that alternate for `--rounds` rounds so that drift and other tenants hit every arm; a
figure is device-event time per call over `--reps` back-to-back calls after `--warmup` calls; each line gives the mean over rounds
with the fastest and slowest round behind it.

  one attention launch   B = 2, H = 8, D = 40, 6144 queries, two segments of 6144 keys per image (the level-0 shape of a 512x768
                         frame with one reference frame and the previous frame).  `torch.cat` of the two float32 entries +
                         `ops.attention_bnhd` (what the parent does per block) against `ops.attention_bnhd_segments` on float32
                         and on float16 entries, in fp32 and in fp16 arithmetic.  With half entries the parent's path also widens
                         them (`.to(float32)`) before the cat, as `_reference_kv` did.
  one v1.5 forward       `UNetModel.forward_nhwc`, SD v1.5 configuration, seeded weights, batch 2 on a 64x96 latent, two reference
                         frames in "all" mode (the histories of two earlier forwards), `--precision` / `--attention-precision`
                         (default fp16 / fp16).  Arms: `parent` -- the package and library of the parent commit, found under
                         --baseline-root (a checkout of the parent with its library built; its float32 history); `fp32` -- this
                         tree, kv_dtype="fp32"; `fp16` -- this tree, kv_dtype="fp16", the references fed as the half histories
                         it records; `concat` -- this tree with OFX_ST_KV_CONCAT=1 (the parent's path inside this library).
                         Per arm: ms per forward, torch.cuda.max_memory_allocated over the timed forwards, and the byte size of
                         one pickled history.

    python tools/kv_history_rate.py --baseline-root ../parent [--out profiles/r38_kv_history_rate.txt]
"""
import argparse
import json
import os
import pickle
import subprocess
import sys

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, LAT_H, LAT_W, CTX_TOKENS = 2, 64, 96, 77
ATT = dict(B=2, H=8, D=40, Nq=6144, n=6144)


def _timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def child_attention(reps: int, warmup: int) -> None:
    import torch
    from sd_animation_optical_flow_amd import ops
    B, H, D, Nq, n = (ATT[k] for k in ("B", "H", "D", "Nq", "n"))
    g = torch.Generator().manual_seed(1)
    q = torch.randn((B, Nq, H * D), generator=g).cuda()
    ents = [(torch.randn((B, n, H * D), generator=g).cuda(), torch.randn((B, n, H * D), generator=g).cuda()) for _ in range(2)]
    half = [(k.half(), v.half()) for k, v in ents]
    res = {}
    for prec in ("fp32", "fp16"):
        def cat32():
            return ops.attention_bnhd(q, torch.cat([e[0] for e in ents], 1), torch.cat([e[1] for e in ents], 1), H, precision=prec)

        def cat16():            # the parent's way with a half history: widen every entry, then join
            return ops.attention_bnhd(q, torch.cat([e[0].to(torch.float32) for e in half], 1),
                                      torch.cat([e[1].to(torch.float32) for e in half], 1), H, precision=prec)

        seg = lambda es: ops.attention_bnhd_segments(q, [[(k[b], v[b]) for k, v in es] for b in range(B)], H, precision=prec)
        a, b = cat32(), seg(ents)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "segments differ from the concatenation"
        res[prec] = {"cat_f32": _timed(cat32, reps, warmup), "seg_f32": _timed(lambda: seg(ents), reps, warmup),
                     "cat_f16": _timed(cat16, reps, warmup), "seg_f16": _timed(lambda: seg(half), reps, warmup)}
    print("RESULT " + json.dumps(res))


def child_forward(arm: str, reps: int, warmup: int, precision: str, attention_precision: str) -> None:
    import torch
    from sd_animation_optical_flow_amd import unet as UN
    cfg = UN.SD_V15_UNET
    kw = {} if arm in ("parent", "concat") else {"kv_dtype": arm}
    model = UN.UNetModel(UN.random_unet_state_dict(0, cfg), cfg, prefix="", precision=precision, attention_precision=attention_precision, **kw)
    g = torch.Generator().manual_seed(20)
    x = torch.randn((BATCH, LAT_H, LAT_W, cfg["in_channels"]), generator=g).cuda()
    x2 = torch.randn((BATCH, LAT_H, LAT_W, cfg["in_channels"]), generator=g).cuda()
    t = torch.tensor([981.0, 981.0]).cuda()
    ctx = torch.randn((BATCH, CTX_TOKENS, cfg["context_dim"]), generator=g).cuda()
    _, kv1 = model.forward_nhwc(x, t, ctx)
    _, kv2 = model.forward_nhwc(x2, t, ctx)
    refs = [kv1, kv2]
    out, hist = model.forward_nhwc(x, t, ctx, reference_kv=refs)
    res = {"arm": arm, "checksum": float(out.double().abs().mean()), "hist_dtype": str(hist[0][0].dtype),
           "hist_bytes": sum(k.numel() * k.element_size() + v.numel() * v.element_size() for k, v in hist),
           "pickle_bytes": len(pickle.dumps([(k.cpu(), v.cpu()) for k, v in hist], protocol=pickle.HIGHEST_PROTOCOL))}
    del out, hist
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res["ms"] = _timed(lambda: model.forward_nhwc(x, t, ctx, reference_kv=refs), reps, warmup)
    res["peak_bytes"] = torch.cuda.max_memory_allocated()
    res["resident_bytes"] = base                                   # weights, inputs and the two reference histories
    print("RESULT " + json.dumps(res))


def _spawn(args, root, env_extra):
    env = dict(os.environ, **env_extra)
    env["OFX_KV_RATE_ROOT"] = root
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + args, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(f"child {args} failed ({r.returncode}); nothing further is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    print(f"done: {' '.join(args[:2])}", file=sys.stderr, flush=True)
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--attention-precision", default="fp16")
    ap.add_argument("--baseline-root", help="a checkout of the parent commit with its library built; without it the `parent` arm is left out")
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--child", nargs="+")
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, os.environ.get("OFX_KV_RATE_ROOT") or HERE_ROOT)
        import torch
        assert torch.cuda.is_available(), "a GPU is needed: nothing here is measured on the host"
        if a.child[0] == "attention":
            child_attention(a.reps, a.warmup)
        else:
            child_forward(a.child[1], a.reps, a.warmup, a.precision, a.attention_precision)
        return
    common = ["--reps", str(a.reps), "--warmup", str(a.warmup), "--precision", a.precision, "--attention-precision", a.attention_precision]
    stat = lambda v: f"{sum(v) / len(v):8.3f} [{min(v):7.3f} .. {max(v):7.3f}]"
    arms = (["parent"] if a.baseline_root else []) + ["fp32", "fp16", "concat"]
    att, fwd = [], {arm: [] for arm in arms}
    for rnd in range(a.rounds):
        att.append(_spawn(["attention"] + common, HERE_ROOT, {}))
        if a.skip_forward:
            continue
        for arm in arms:
            root = os.path.abspath(a.baseline_root) if arm == "parent" else HERE_ROOT
            fwd[arm].append(_spawn(["forward", arm] + common, root, {"OFX_ST_KV_CONCAT": "1"} if arm == "concat" else {"OFX_ST_KV_CONCAT": "0"}))
    B, H, D, Nq, n = (ATT[k] for k in ("B", "H", "D", "Nq", "n"))
    lines = [f"One attention launch: B {B}, H {H}, D {D}, {Nq} queries, two entries of {n} keys per image; ms per call, device events over "
             f"{a.reps} calls, mean of {a.rounds} rounds [fastest .. slowest].  cat = torch.cat of the entries (half entries widened first) + "
             f"ops.attention_bnhd, the parent's path; segments = ops.attention_bnhd_segments on the entries where they lie.", ""]
    for prec in ("fp32", "fp16"):
        for kvt in ("f32", "f16"):
            c, s = [r[prec]["cat_" + kvt] for r in att], [r[prec]["seg_" + kvt] for r in att]
            lines.append(f"  arithmetic {prec}, K/V {'float32' if kvt == 'f32' else 'float16'}:  cat {stat(c)}   segments {stat(s)}   cat / segments = "
                         f"{sum(c) / sum(s):.3f}")
    if not a.skip_forward:
        lines += ["", f"UNetModel.forward_nhwc(precision={a.precision!r}, attention_precision={a.attention_precision!r}), SD v1.5 configuration, "
                      f"seeded weights, batch {BATCH}, latent {LAT_H} x {LAT_W}, context {CTX_TOKENS} x 768, two reference frames in \"all\" mode; "
                      f"ms per forward, device events over {a.reps} forwards, mean of {a.rounds} rounds [fastest .. slowest]", ""]
        for arm in arms:
            rs = fwd[arm]
            what = {"parent": "parent commit (package and library)", "fp32": "this change, kv_dtype fp32", "fp16": "this change, kv_dtype fp16",
                    "concat": "this change, OFX_ST_KV_CONCAT=1"}[arm]
            lines.append(f"  {what:38s} {stat([r['ms'] for r in rs])} ms   peak allocated {max(r['peak_bytes'] for r in rs) / 1e6:8.1f} MB "
                         f"(resident before the forward {rs[0]['resident_bytes'] / 1e6:8.1f} MB)   one history {rs[0]['hist_bytes'] / 1e6:7.1f} MB "
                         f"{rs[0]['hist_dtype']}, pickled {rs[0]['pickle_bytes'] / 1e6:7.1f} MB   mean |out| {rs[0]['checksum']:.6f}")
        if "parent" in fwd:
            p, m = [r["ms"] for r in fwd["parent"]], [r["ms"] for r in fwd["fp32"]]
            h = [r["ms"] for r in fwd["fp16"]]
            lines.append(f"  parent / fp32 = {sum(p) / sum(m):.3f}, parent / fp16 = {sum(p) / sum(h):.3f}; the brackets "
                         f"{'overlap or lie below' if min(m) <= max(p) and min(h) <= max(p) else 'LIE ABOVE'} the parent's")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
