"""Time `ops.attention` on the UNet's self-/cross-attention shapes on the GPU box.

    python tools/attn_bench.py
        the shapes at 1024x1024 (latent 128x128), fp32, one process: ms and TFLOP/s (4 * BH * Nq * Nk * D flops) per shape; the D = 48
        rows run the unfused path for comparison.
    python tools/attn_bench.py --precision fp32,fp16 [--shapes unet] [--rounds 3] [--out profiles/r24_attn_f16_rate.txt]
        A/B of `ops.attention(precision=)`: every precision in a fresh process of its own, the precisions alternating for `--rounds`
        rounds of one session; per shape the mean over the rounds with [fastest .. slowest] and, against the first precision named,
        the ratio and whether the brackets overlap.  `--shapes unet`: the SD v1.5 UNet's own shapes at batch 2 on a 64 x 96 latent
        (self-attention of its four levels, each level's cross-attention against 77 context tokens) and the 16384-token shape.
A figure is device-event time per call over `--reps` back-to-back calls after `--warmup` calls.  The unfused D = 48 rows exist in fp32
only and are left out of an A/B that names "fp16"."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    "1024": [("level0 self", 8, 16384, 16384, 40), ("level0 self x2 (cfg)", 16, 16384, 16384, 40), ("level0 cross", 16, 16384, 77, 40),
             ("level1 self", 16, 4096, 4096, 80), ("level2 self", 16, 1024, 1024, 160), ("level0 kv-history x3", 8, 16384, 49152, 40),
             ("512^2 level0 self", 16, 4096, 4096, 40), ("unfused d=48", 8, 8192, 8192, 48), ("fused d=40 same", 8, 8192, 8192, 40)],
    "unet": [("level0 self 6144", 16, 6144, 6144, 40), ("level1 self 1536", 16, 1536, 1536, 80), ("level2 self 384", 16, 384, 384, 160),
             ("mid self 96", 16, 96, 96, 160), ("level0 cross 6144x77", 16, 6144, 77, 40), ("level1 cross 1536x77", 16, 1536, 77, 80),
             ("level2 cross 384x77", 16, 384, 77, 160), ("mid cross 96x77", 16, 96, 77, 160), ("16384 tokens x 8 heads", 8, 16384, 16384, 40)],
}
FUSED = (40, 64, 80, 128, 160)


def child(shapes, precision, reps, warmup):
    import torch
    from sd_animation_optical_flow_amd import ops
    assert torch.cuda.is_available(), "a GPU is needed: nothing here is measured on the host"
    res = {}
    for name, BH, Nq, Nk, D in shapes:
        g = torch.Generator(device="cuda").manual_seed(1)
        q = torch.randn((BH, Nq, D), device="cuda", generator=g)
        k = torch.randn((BH, Nk, D), device="cuda", generator=g)
        v = torch.randn((BH, Nk, D), device="cuda", generator=g)
        for _ in range(warmup):
            o = ops.attention(q, k, v, precision=precision)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            o = ops.attention(q, k, v, precision=precision)
        e1.record()
        torch.cuda.synchronize()
        res[name] = {"ms": e0.elapsed_time(e1) / reps, "checksum": float(o.double().abs().mean())}
        del q, k, v, o
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp32", help="comma-separated ops.attention precisions, the baseline first (fp32,fp16)")
    ap.add_argument("--shapes", default="1024", choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out")
    ap.add_argument("--child")
    a = ap.parse_args()
    precs = [p.strip() for p in a.precision.split(",") if p.strip()]
    shapes = [s for s in SHAPES[a.shapes] if s[4] in FUSED or precs == ["fp32"]]
    if a.child:
        child(shapes, a.child, a.reps, a.warmup)
        return
    runs = {p: [] for p in precs}
    for rnd in range(a.rounds):
        for p in precs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", p, "--precision", a.precision, "--shapes", a.shapes, "--reps", str(a.reps),
                   "--warmup", str(a.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
            if r.returncode != 0:
                sys.exit(f"child failed ({r.returncode}); nothing further is started\n{r.stdout}\n{r.stderr}")
            runs[p].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
            print(f"round {rnd} {p} done", flush=True)
    stat = lambda v: f"{sum(v) / len(v):9.3f} [{min(v):8.3f} .. {max(v):8.3f}]"
    lines = [f"ops.attention(precision=), ms per call: device events over {a.reps} calls after {a.warmup} warm-up, mean of {a.rounds} rounds "
             f"[fastest .. slowest], the precisions in alternating fresh processes of one session; TFLOP/s = 4 BH Nq Nk D / mean", ""]
    base = precs[0]
    for name, BH, Nq, Nk, D in shapes:
        lines.append(f"{name}: BH={BH} Nq={Nq} Nk={Nk} D={D}")
        ms = {p: [r[name]["ms"] for r in runs[p]] for p in precs}
        for p in precs:
            mean = sum(ms[p]) / len(ms[p])
            line = f"  {p:5s} {stat(ms[p])} ms  {4.0 * BH * Nq * Nk * D / mean / 1e9:7.1f} TFLOP/s  mean |out| {runs[p][0][name]['checksum']:.6f}"
            if p != base:
                clear = max(ms[p]) < min(ms[base]) or min(ms[p]) > max(ms[base])
                line += f"   {base} / {p} = {sum(ms[base]) / sum(ms[p]):.3f} ({'brackets apart' if clear else 'BRACKETS OVERLAP'})"
            lines.append(line)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
