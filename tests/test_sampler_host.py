"""CPU: the sampler's host side against tests/golden/sampler_ref_u0.npz, the output of the reference's own DDIMSampler and UNet
(tests/golden/make_golden_sampler.py): the schedule tables bit for bit, the loop's bookkeeping, the float64 restatement that the GPU
tests measure against, and every refusal that must come before a device is touched."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import sampler_check as SK
import transformer_check as TC
import unet_check as UC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sampler_ref_u0.npz")
TABLES = ("ddim_timesteps", "ddim_alphas", "ddim_alphas_prev", "ddim_sigmas", "ddim_sqrt_one_minus_alphas", "sqrt_alphas_cumprod",
          "sqrt_one_minus_alphas_cumprod")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _inputs(gold):
    return {k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("in.")}


def test_import_needs_no_device():
    code = ("import sys, torch; torch.cuda.is_available = lambda: False\n"
            "import sd_animation_optical_flow_amd.sampler as s\n"
            "assert len(s.ddim_schedule(50)['ddim_timesteps']) == 50\n"
            "assert not torch.cuda.is_initialized()\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", PYTHONPATH=ROOT)
    subprocess.run([sys.executable, "-s", "-c", code], check=True, env=env, cwd=ROOT)


@pytest.mark.parametrize("steps,eta", SK.SCHEDULES)
def test_ddim_schedule_is_the_reference_tables_bit_for_bit(gold, steps, eta):
    from sd_animation_optical_flow_amd.sampler import ddim_schedule
    s = ddim_schedule(steps, eta)
    for n in TABLES:
        want, got = gold[f"sched_{steps}_{eta}.{n}"], s[n]
        kind = str(gold[f"sched_{steps}_{eta}.{n}.kind"]) if f"sched_{steps}_{eta}.{n}.kind" in gold.files else "tensor"
        assert (kind == "tensor") == torch.is_tensor(got), f"{n}: the reference holds a {kind}"
        arr = got.numpy() if torch.is_tensor(got) else got
        assert arr.dtype == want.dtype, f"{n}: dtype {arr.dtype}, the reference's is {want.dtype}"
        assert arr.shape == want.shape and arr.tobytes() == want.tobytes(), f"{n} differs from the reference"
    # the mixture the docstring names
    assert s["ddim_alphas"].dtype == torch.float32 and isinstance(s["ddim_alphas_prev"], np.ndarray)
    assert s["ddim_alphas_prev"].dtype == np.float64 and s["ddim_sigmas"].dtype == torch.float64
    assert (float(s["ddim_sigmas"].abs().max()) > 0) == (eta > 0)


def test_schedule_refusals():
    from sd_animation_optical_flow_amd.sampler import ddim_schedule
    with pytest.raises(NotImplementedError):
        ddim_schedule(10, beta_schedule="cosine")
    with pytest.raises(NotImplementedError):
        ddim_schedule(10, ddim_discretize="quad")
    with pytest.raises(ValueError):
        ddim_schedule(0)
    with pytest.raises(ValueError):
        ddim_schedule(1000)                 # the last step would index alphas_cumprod[1000]


@pytest.mark.parametrize("name", sorted(SK.DECODE_CASES))
def test_bookkeeping_is_the_reference_loop(gold, name):
    from sd_animation_optical_flow_amd.sampler import ddim_schedule, decode_plan
    case = SK.DECODE_CASES[name]
    plan = decode_plan(ddim_schedule(case["steps"], case["eta"]), case["t_start"], case["func"])
    want = gold[f"{name}.plan"]
    assert len(plan) == len(want) == case["t_start"]
    for (p, index, step, gs), w in zip(plan, want):
        assert (p, float(index), float(step), float(gs)) == tuple(w)
    assert float(plan[-1][3]) == float(gold[f"{name}.last_gs"])
    # the reassigned total_steps: p ends at 1 and index at 0 whatever the schedule's length
    assert plan[-1][0] == 1.0 and plan[-1][1] == 0 and plan[0][1] == case["t_start"] - 1


@pytest.mark.parametrize("name", sorted(SK.DECODE_CASES))
def test_float64_restatement_is_the_reference_loop(gold, name):
    """The restatement the GPU test measures against lies within the stored yardstick of the reference's own fp32 result (the
    yardstick is that distance as measured when the file was made; a restatement that drifted would exceed it)."""
    from sd_animation_optical_flow_amd.sampler import ddim_schedule, decode_plan, step_coefficients
    from sd_animation_optical_flow_amd.unet import random_unet_state_dict, unet_layout
    case = SK.DECODE_CASES[name]
    sched = ddim_schedule(case["steps"], case["eta"])
    plan = decode_plan(sched, case["t_start"], case["func"])
    sd64 = TC.to64(random_unet_state_dict(0, UC.U0))
    ref = SK.loop64(sd64, unet_layout(UC.U0), sched, case, _inputs(gold), torch.from_numpy(gold["x1"]), plan,
                    lambda index: step_coefficients(sched, index))
    yard = dict(zip([str(k) for k in gold["dist_keys"]], gold["ref_vs_f64"]))[name]
    d = float((torch.from_numpy(gold[f"{name}.out"]).double() - ref).abs().max())
    print(f"case {name}: reference fp32 vs float64 restatement {d:.3e}, stored yardstick {yard:.3e}")
    assert 0 < yard < 1e-4 * float(np.abs(gold[f"{name}.out"]).max())          # fp32 noise, not a different loop
    assert d <= yard * (1 + 1e-6) + 1e-12


def test_stored_inputs_are_the_seeded_ones(gold):
    inp = SK.decode_inputs()
    for k, v in inp.items():
        assert np.array_equal(gold[f"in.{k}"], v.numpy()), k
    m = gold["in.nmask"]
    assert set(np.unique(m)) == {0.0, 1.0} and (m[:, :, 0] == 0).all() and (m[:, :, 1] == 1).all()
    assert gold["in.c_concat"].shape[1] == 5 and gold["in.context"].shape[1] == 9 and m.shape[2:] == (8, 12)


def _stub_unet():
    return types.SimpleNamespace(in_channels=9, out_channels=4, in_pad=12, cfg=dict(context_dim=64), device=torch.device("cpu"))


@pytest.mark.parametrize("kw", [dict(use_original_steps=True), dict(score_corrector=object()), dict(quantize_denoised=True),
                                dict(noise_dropout=0.1), dict(dynamic_threshold=0.5), dict(guidance_space="pixel"),
                                dict(guidance_schedule_func=lambda p: np.ones((4, 4), np.float32))])
def test_decode_refuses_what_is_not_built_without_a_device(kw):
    from sd_animation_optical_flow_amd.sampler import GuidedDDIMSampler
    s = GuidedDDIMSampler(_stub_unet())
    s.make_schedule(10)
    x = torch.zeros((1, 4, 8, 12))
    with pytest.raises(NotImplementedError):
        s.decode(x, torch.zeros((1, 9, 64)), 4, **kw)


def test_other_refusals_without_a_device():
    from sd_animation_optical_flow_amd.sampler import GuidedDDIMSampler, img2img_inpaint
    with pytest.raises(NotImplementedError):
        GuidedDDIMSampler(_stub_unet(), parameterization="v")
    s = GuidedDDIMSampler(_stub_unet())
    with pytest.raises(RuntimeError, match="make_schedule"):
        s.decode(torch.zeros((1, 4, 8, 12)), torch.zeros((1, 9, 64)), 4)
    s.make_schedule(10)
    with pytest.raises(NotImplementedError):
        s.stochastic_encode(torch.zeros((1, 4, 8, 12)), 4, torch.zeros((1, 4, 8, 12)), use_original_steps=True)
    for t_start in (0, 11, 2.5):
        with pytest.raises(ValueError):
            s.decode(torch.zeros((1, 4, 8, 12)), torch.zeros((1, 9, 64)), t_start)
    with pytest.raises(ValueError):
        s.stochastic_encode(torch.zeros((1, 4, 8, 12)), 10, torch.zeros((1, 4, 8, 12)))
    with pytest.raises(RuntimeError, match="CUDA float32"):                    # a host latent is refused before any launch
        s.decode(torch.zeros((1, 4, 8, 12)), torch.zeros((1, 9, 64)), 4)
    img = np.zeros((64, 96, 3), np.uint8)
    with pytest.raises(NotImplementedError):                                    # the PIL-blur fill_mask_input path
        img2img_inpaint(_stub_unet(), None, None, img, None, img[..., 0], None, None)
    with pytest.raises(ValueError, match="t_enc"):                              # int(0.05 * 10) == 0
        img2img_inpaint(_stub_unet(), None, None, img, img, img[..., 0], None, None, denoising_strength=0.05, ddim_steps=10)


def test_step_coefficients_are_fp32_values():
    from sd_animation_optical_flow_amd.sampler import ddim_schedule, step_coefficients
    s = ddim_schedule(10, 0.5)
    k = step_coefficients(s, 3, temperature=0.5)
    for v in k.values():
        assert float(np.float32(v)) == v
    a, ap, sg = np.float32(s["ddim_alphas"][3]), np.float32(s["ddim_alphas_prev"][3]), np.float32(float(s["ddim_sigmas"][3]))
    assert k["sqrt_at"] == float(np.sqrt(a)) and k["sqrt_aprev"] == float(np.sqrt(ap))
    assert k["dir_coef"] == float(np.sqrt(np.float32(1.0) - ap - sg * sg)) and k["sigma_t"] == float(sg * np.float32(0.5))
