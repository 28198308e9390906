"""A/B of `ops.groupnorm` between two builds of the library on the GPU box.

    python tools/groupnorm_ab.py --libs parent=tools/variants/libofx_parent.so,new= [--rounds 3] [--out profiles/groupnorm_fold_ab.txt]

Every build (name=path, the baseline first; an empty path is the in-tree library) runs in a fresh process of its own (OFX_LIB_PATH),
the builds alternating for `--rounds` rounds of one session -- the procedure of tools/attn_bench.py.  Shapes: the VAE decoder's
GroupNorm + SiLU at a 512 x 768 frame (B = 1, 32 groups) and the transformer's entry norm (B = 2, 64 x 96, C = 320, no SiLU).  A figure
is device-event time per call over `--reps` back-to-back calls after `--warmup` calls; per shape the mean over the rounds with
[fastest .. slowest] and, against the baseline, the ratio and whether the brackets overlap."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name, B, H, W, C, groups, silu
SHAPES = [("vae 64x96 c512", 1, 64, 96, 512, 32, True), ("vae 128x192 c512", 1, 128, 192, 512, 32, True),
          ("vae 256x384 c256", 1, 256, 384, 256, 32, True), ("vae 512x768 c128", 1, 512, 768, 128, 32, True),
          ("transformer entry 64x96 c320", 2, 64, 96, 320, 32, False)]


def child(reps, warmup):
    import torch
    from sd_animation_optical_flow_amd import _lib, ops
    assert torch.cuda.is_available(), "a GPU is needed: nothing here is measured on the host"
    res = {"lib": _lib.LIB_PATH}
    for name, B, H, W, C, groups, silu in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn((B, H, W, C), device="cuda", generator=g)
        gamma = torch.randn((C,), device="cuda", generator=g)
        beta = torch.randn((C,), device="cuda", generator=g)
        out = torch.empty_like(x)
        scratch = torch.empty((_lib.lib().ofx_groupnorm_scratch_bytes(B, C),), dtype=torch.uint8, device="cuda")
        for _ in range(warmup):
            ops.groupnorm(x, gamma, beta, groups, 1e-6, silu, out=out, scratch=scratch)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            ops.groupnorm(x, gamma, beta, groups, 1e-6, silu, out=out, scratch=scratch)
        e1.record()
        torch.cuda.synchronize()
        res[name] = {"ms": e0.elapsed_time(e1) / reps, "checksum": float(out.double().abs().mean())}
        del x, out, scratch
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default="new=", help="comma-separated name=path builds, the baseline first; an empty path: the in-tree library")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.reps, a.warmup)
        return
    libs = [tuple(s.split("=", 1)) for s in a.libs.split(",")]
    runs = {n: [] for n, _ in libs}
    for rnd in range(a.rounds):
        for n, path in libs:
            env = dict(os.environ)
            env.pop("OFX_LIB_PATH", None)
            if path:
                env["OFX_LIB_PATH"] = os.path.abspath(path)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup", str(a.warmup)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"child failed ({r.returncode}); nothing further is started\n{r.stdout}\n{r.stderr}")
            runs[n].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
            print(f"round {rnd} {n} done", flush=True)
    stat = lambda v: f"{sum(v) / len(v):9.4f} [{min(v):8.4f} .. {max(v):8.4f}]"
    lines = [f"ops.groupnorm, ms per call: device events over {a.reps} calls after {a.warmup} warm-up, mean of {a.rounds} rounds [fastest .. "
             f"slowest], the builds in alternating fresh processes of one session", ""]
    base = libs[0][0]
    for name, B, H, W, C, groups, silu in SHAPES:
        lines.append(f"{name}: B={B} HW={H}x{W} C={C} groups={groups} silu={int(silu)}")
        ms = {n: [r[name]["ms"] for r in runs[n]] for n, _ in libs}
        for n, _ in libs:
            line = f"  {n:8s} {stat(ms[n])} ms  mean |out| {runs[n][0][name]['checksum']:.9f}"
            if n != base:
                apart = max(ms[n]) < min(ms[base]) or min(ms[n]) > max(ms[base])
                verdict = "brackets overlap" if not apart else ("below the baseline's" if max(ms[n]) < min(ms[base]) else "ABOVE THE BASELINE'S")
                line += f"   {n} / {base} = {sum(ms[n]) / sum(ms[base]):.3f} ({verdict})"
            lines.append(line)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
