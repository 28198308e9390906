#!/usr/bin/env python3
"""CLIP text encoder rate on the full SD v1.5 configuration: one `ClipTextEncoder.conditioning` call (prompt and negative prompt,
tokens on the host in, the two [1,231,768] context tensors on the device out) for a short prompt pair (three distinct 77-token
sequences of the six) and a long one (six distinct), with `dedupe` on and off, against the same forward written from torch ops on
the device (F.embedding, F.layer_norm, F.linear, scaled_dot_product_attention with the causal mask, x * sigmoid(1.702 x)); and the
two kernels of csrc/text_encoder.hip against their torch expressions at the production shapes.

Workload: `SD_V15_CLIP_TEXT` with seeded weights, clip_skip 0.  The reference computes both tensors once per `img2img*` call
(guided_ldm_inpainting.py:200-203), i.e. once per frame, so none of this is on the sampler's per-step path: the figures are
recorded, not gated.

One process; after `--warmup` calls of everything, `--rounds` rounds in which the variants alternate (so that drift and other
tenants hit all of them), each timing `--reps` back-to-back calls between two device events (the host work of a call -- the
dedupe, the copy of the tokens -- is inside the window).  A figure is the median over rounds with the fastest and slowest round
behind it.

    python tools/text_encoder_rate.py [--out profiles/r28_text_encoder_rate.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOS, EOS, PAD = 49406, 49407, 49407
KERNEL_ROWS = 6 * 77


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from sd_animation_optical_flow_amd import ops, text_encoder as TE
    assert torch.cuda.is_available(), "a GPU is needed: nothing here is measured on the host"
    cfg = TE.SD_V15_CLIP_TEXT
    W, H, L = cfg["width"], cfg["heads"], cfg["layers"]
    sd = TE.random_clip_text_state_dict(0, cfg)
    enc = {dd: TE.ClipTextEncoder(sd, cfg, prefix="", dedupe=dd) for dd in (True, False)}
    assert not enc[True].torch_glue, "unset OFX_CLIP_TORCH_GLUE: the tool times the torch forward itself"
    dw = {k: v.cuda() for k, v in sd.items()}
    causal = torch.full((77, 77), float("-inf")).triu(1).cuda()

    def torch_forward(tokens):
        """The same forward from torch ops: tokens [B,3,77] on the host -> [B,231,768]."""
        B = tokens.shape[0]
        ids = tokens.reshape(-1, 77).to("cuda", non_blocking=True).long()
        S = ids.shape[0]
        x = F.embedding(ids, dw["embeddings.token_embedding.weight"]) + dw["embeddings.position_embedding.weight"]
        for i in range(L):
            l = f"encoder.layers.{i}"
            h = F.layer_norm(x, (W,), dw[f"{l}.layer_norm1.weight"], dw[f"{l}.layer_norm1.bias"], 1e-5)
            q, k, v = (F.linear(h, dw[f"{l}.self_attn.{n}.weight"], dw[f"{l}.self_attn.{n}.bias"]).view(S, 77, H, W // H).transpose(1, 2)
                       for n in ("q_proj", "k_proj", "v_proj"))
            o = F.scaled_dot_product_attention(q, k, v, attn_mask=causal).transpose(1, 2).reshape(S, 77, W)
            x = x + F.linear(o, dw[f"{l}.self_attn.out_proj.weight"], dw[f"{l}.self_attn.out_proj.bias"])
            m = F.linear(F.layer_norm(x, (W,), dw[f"{l}.layer_norm2.weight"], dw[f"{l}.layer_norm2.bias"], 1e-5),
                         dw[f"{l}.mlp.fc1.weight"], dw[f"{l}.mlp.fc1.bias"])
            x = x + F.linear(m * torch.sigmoid(1.702 * m), dw[f"{l}.mlp.fc2.weight"], dw[f"{l}.mlp.fc2.bias"])
        x = F.layer_norm(x, (W,), dw["final_layer_norm.weight"], dw["final_layer_norm.bias"], 1e-5)
        return x.view(B, 231, W)

    def torch_conditioning(tc, tu):
        both = torch_forward(torch.cat([tc, tu]))
        return both[:1], both[1:]

    g = torch.Generator().manual_seed(28)
    ids = lambda n: torch.randint(0, BOS, (n,), generator=g).tolist()
    pairs = {"short pair (12 + 7 ids: 3 distinct sequences)": (ids(12), ids(7)),
             "long pair (200 + 160 ids: 6 distinct sequences)": (ids(200), ids(160))}
    variants, groups = [], []
    for label, (c, uc) in pairs.items():
        tc, tu = TE.chunk_tokens([c], BOS, EOS, PAD), TE.chunk_tokens([uc], BOS, EOS, PAD)
        ref = torch_conditioning(tc, tu)
        for dd in (True, False):                                   # the two really compute the same tensors
            got = enc[dd].conditioning(tc, tu)
            err = max(float((x - y).abs().max()) for x, y in zip(got, ref))
            assert err <= 1e-3, (label, dd, err)
        names = [f"{label}: conditioning, dedupe on", f"{label}: conditioning, dedupe off", f"{label}: torch ops"]
        variants += [(names[0], lambda tc=tc, tu=tu: enc[True].conditioning(tc, tu)),
                     (names[1], lambda tc=tc, tu=tu: enc[False].conditioning(tc, tu)),
                     (names[2], lambda tc=tc, tu=tu: torch_conditioning(tc, tu))]
        groups.append((label, names, enc[True].embed_rows // 77))
    # the two kernels against their torch expressions
    kid = torch.randint(0, BOS, (KERNEL_ROWS,), generator=g).to(torch.int32).cuda()
    kid64 = kid.long()
    tok, pos = enc[True].tok, enc[True].pos
    pos_rows = pos.repeat(KERNEL_ROWS // 77, 1)
    kernels = [(f"clip_embed {KERNEL_ROWS} x {W}", lambda: ops.clip_embed(kid, tok, pos, 77), lambda: F.embedding(kid64, tok) + pos_rows)]
    for n in (W, cfg["intermediate"]):
        xq = torch.randn((KERNEL_ROWS, n), generator=g).cuda()
        kernels.append((f"quick_gelu {KERNEL_ROWS} x {n}", lambda xq=xq: ops.quick_gelu(xq), lambda xq=xq: xq * torch.sigmoid(1.702 * xq)))
    for name, kf, tf in kernels:
        assert float((kf() - tf()).abs().max()) <= 1e-5, name
        variants += [(f"{name} kernel", kf), (f"{name} torch", tf)]

    for _, fn in variants:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {label: [] for label, _ in variants}
    for _ in range(a.rounds):
        for label, fn in variants:
            reps = a.reps * (20 if " x " in label else 1)         # a single elementwise launch: more calls per window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[label].append(e0.elapsed_time(e1) / reps)

    def fig(label):
        v = times[label]
        return statistics.median(v), min(v), max(v)

    lines = [f"CLIP text encoder rate: SD_V15_CLIP_TEXT ({L} layers, width {W}, {H} heads), seeded weights, clip_skip 0, one prompt and one "
             "negative prompt per call",
             f"device: {torch.cuda.get_device_name(0)}; one process, {a.warmup} warm-up calls, {a.rounds} alternating rounds of {a.reps} "
             "back-to-back calls (x 20 for the single kernels); ms per call: median over rounds [fastest, slowest]", ""]
    for label, names, distinct in groups:
        lines.append(f"{label}; the transformer sees {distinct} sequences with dedupe, 6 without")
        base = fig(names[2])[0]
        for nm in names:
            m, lo, hi = fig(nm)
            lines.append(f"  {nm.rsplit(': ', 1)[1]:28s} {m:9.3f} ms [{lo:.3f}, {hi:.3f}]   / torch ops {m / base:5.2f}")
        lines.append("")
    lines.append("the kernels of csrc/text_encoder.hip against their torch expressions (F.embedding + add; x * sigmoid(1.702 x))")
    losses = []
    for name, _, _ in kernels:
        k, kl, kh = fig(f"{name} kernel")
        t, tl, th = fig(f"{name} torch")
        lines.append(f"  {name:24s} kernel {k * 1e3:8.1f} us [{kl * 1e3:.1f}, {kh * 1e3:.1f}]   torch {t * 1e3:8.1f} us [{tl * 1e3:.1f}, {th * 1e3:.1f}]   "
                     f"kernel / torch {k / t:5.2f}")
        if k > t:
            losses.append(name)
    lines.append("  the kernel loses to the torch expression on: " + (", ".join(losses) if losses else "no shape"))
    slower = [nm for _, names, _ in groups for nm in names[:2] if fig(nm)[0] > fig(names[2])[0]]
    lines.append("conditioning is slower than the torch composition on: " + ("; ".join(slower) if slower else "no variant"))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
