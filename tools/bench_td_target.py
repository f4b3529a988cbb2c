"""The fused TD target (FusedTDTarget: one k_target_pack launch per refresh, one k_td_target launch per target) against the
eager torch ``no_grad`` block of SB3's SAC.train / TD3.train on the same modules and batch.

    python tools/bench_td_target.py [--reps 50] [--out FILE]

For SAC (ReLU [128, 128, 128]) and TD3 (ReLU [256, 256]) at B = 100, 256, 4096, 65 536: the median milliseconds of `reps`
CUDA-event pairs after a warm-up call of (a) td.refresh(); td.target(samples, seed, counter), (b) td.target alone, (c) the
eager block (its noise drawn by torch.randn_like inside the timed region, as SB3 does).  Host overhead and output allocation
are included on both sides.  Before anything is timed the fused target fed the eager block's eps is asserted to lie within
2 x bound of it elementwise (tests/td_target_ref.py; both sides within bound of fp64).  One JSON line per shape, with the
f32 MFMA rate (b) implies -- the flops of the tiles the kernel issues, padding included: 233 472 per sample for SAC, 466 944
for TD3 -- against the 157.3 TFLOP/s peak.  The gate: at every shape the median of (a), refresh included, is not above the
eager median (c); the exit status is 1 otherwise.  Then a summary line with the library's source hash
(tools/source_state.py).  Kernel durations come from a rocprofv3 --kernel-trace --stats run of this script."""
import argparse
import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

BATCHES = [100, 256, 4096, 65536]
GAMMA = 0.99
MFMA_FLOP_PER_SAMPLE = {"sac": 3 * 2 * (32 * 128 + 2 * 128 * 128 + 128 * 16), "td3": 3 * 2 * (32 * 256 + 256 * 256 + 256 * 16)}
PEAK_F32_MFMA = 157.3e12


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def eager_block(torch, mc, s, eps, ent_coef):
    """SB3's statements on stand-in modules; eps None: drawn here, as SAC's rsample / TD3's normal_ do."""
    relu = torch.relu

    def mlp(layers, x):
        for l in layers[:-1]:
            x = relu(l(x))
        return layers[-1](x)

    with torch.no_grad():
        obs = s.next_observations
        if mc["kind"] == "sac":
            latent = obs
            for l in mc["lin"]:
                latent = relu(l(latent))
            mean, log_std = mc["mu"](latent), torch.clamp(mc["ls"](latent), -20, 2)
            std = log_std.exp()
            gaussian = mean + std * (eps if eps is not None else torch.randn_like(mean))
            next_actions = torch.tanh(gaussian)
            lp = torch.distributions.Normal(mean, std).log_prob(gaussian).sum(dim=1)
            lp -= torch.sum(torch.log(1 - next_actions ** 2 + 1e-6), dim=1)
        else:
            noise = (0.2 * eps) if eps is not None else s.actions.clone().data.normal_(0, 0.2)
            next_actions = (torch.tanh(mlp(mc["lin"] + [mc["mu"]], obs)) + noise.clamp(-0.5, 0.5)).clamp(-1, 1)
        qin = torch.cat([obs, next_actions], dim=1)
        q = torch.cat((mlp(mc["q1"], qin), mlp(mc["q2"], qin)), dim=1)
        q, _ = torch.min(q, dim=1, keepdim=True)
        if mc["kind"] == "sac":
            q = q - ent_coef * lp.reshape(-1, 1)
        return s.rewards + (1 - s.dones) * GAMMA * q


def measure(reps):
    import torch

    import policy_ref as R
    import td_target_ref as T
    from reinforcementlearning4meshgeneration_amd import FusedTDTarget, ReplayBufferSamples
    obs_all = np.ascontiguousarray(np.resize(R.input_rows(), (max(BATCHES), 18)))
    eps_all = R.noise_rows(max(BATCHES))
    rows = []
    for kind in ("sac", "td3"):
        m = T.sac_modules() if kind == "sac" else T.td3_modules()
        mc = {k: ([copy.deepcopy(l).cuda() for l in v] if isinstance(v, list) else (copy.deepcopy(v).cuda() if hasattr(v, "weight") else v))
              for k, v in m.items()}
        lec = torch.tensor([-3.0], dtype=torch.float32, device="cuda") if kind == "sac" else None
        if kind == "sac":
            td = FusedTDTarget.sac(mc["lin"], mc["mu"], mc["ls"], mc["q1"], mc["q2"], GAMMA, log_ent_coef=lec)
            kw = dict(gamma_=GAMMA, log_ent_coef=np.float32(-3.0))
        else:
            td = FusedTDTarget.td3(mc["lin"], mc["mu"], mc["q1"], mc["q2"], GAMMA, policy_noise=0.2, noise_clip=0.5)
            kw = dict(gamma_=GAMMA, policy_noise=0.2, noise_clip=0.5)
        for B in BATCHES:
            obs_np, eps_np = obs_all[:B], eps_all[:B]
            rew_np, done_np = T.batch_rows(B)
            up = lambda x: torch.from_numpy(x).cuda()   # noqa: E731
            s = ReplayBufferSamples(up(obs_np), torch.zeros((B, 3), device="cuda"), up(obs_np), up(done_np).reshape(-1, 1),
                                    up(rew_np).reshape(-1, 1))
            eps = up(eps_np)
            ent = (lambda: torch.exp(lec.detach())) if kind == "sac" else (lambda: None)
            y = td.target(s, noise=eps).cpu().numpy()[:, 0]
            e = eager_block(torch, mc, s, eps, ent()).cpu().numpy()[:, 0]
            ref, bound = T.target_ref(m, obs_np, rew_np, done_np, eps_np, **kw)["target"]
            pair, bad = R.ratio(y, (e.astype(np.float64), 2.0 * bound))
            assert not bad.any(), f"{kind} B={B}: fused and eager differ by more than 2 x bound"
            counter = [0]

            def fused_refresh():
                counter[0] += 1
                td.refresh()
                return td.target(s, seed=3, counter=counter[0])

            def fused_only():
                counter[0] += 1
                return td.target(s, seed=3, counter=counter[0])

            a_ms, b_ms = timed(torch, fused_refresh, reps), timed(torch, fused_only, reps)
            c_ms = timed(torch, lambda: eager_block(torch, mc, s, None, ent()), reps)
            row = dict(kind=kind, B=B, fused_refresh_target_ms=round(a_ms, 4), fused_target_ms=round(b_ms, 4), eager_ms=round(c_ms, 4),
                       eager_over_fused=round(c_ms / a_ms, 2), eager_over_target_alone=round(c_ms / b_ms, 2),
                       fused_minus_eager_over_2bound=round(pair, 4),
                       fused_over_fp64_bound=round(R.ratio(y, (ref, bound))[0], 4), eager_over_fp64_bound=round(R.ratio(e, (ref, bound))[0], 4),
                       mfma_TFLOPs_call=round(B * MFMA_FLOP_PER_SAMPLE[kind] / (b_ms * 1e-3) / 1e12, 3),
                       mfma_fraction_of_peak_call=round(B * MFMA_FLOP_PER_SAMPLE[kind] / (b_ms * 1e-3) / PEAK_F32_MFMA, 4),
                       gate_fused_not_above_eager=bool(a_ms <= c_ms))
            print(json.dumps(row), flush=True)
            rows.append(row)
        td.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from source_state import state
    rows = measure(args.reps)
    ok = all(r["gate_fused_not_above_eager"] for r in rows)
    summary = dict(summary="bench_td_target", **state(), gate_holds_at_every_shape=ok, rows=rows)
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
