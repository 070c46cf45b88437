"""Measurements behind profiles/deterministic.txt (DESIGN.md "Deterministic mode").

    python scratch/det_measure.py sites      per site: the fixed-order form's alone-time beside the atomic form's (median of 20 launches)
    python scratch/det_measure.py scatter    the evidence: per-parameter largest run-to-run difference over five default-mode steps on the
                                             large-row batch of tests/test_deterministic_gpu.py, and the same figure in the mode (0)
    python scratch/det_measure.py steps [bench.py arguments]
                                             bench.py in fresh processes, arms alternated: MMDTI_DETERMINISTIC=0 / 1 (2 rounds)
    python scratch/det_measure.py ab OLD.so NEW.so [bench.py arguments]
                                             the same with two builds of the library through MMDTI_HIP_LIB (old, old, new alternated: the
                                             old-against-old spread is the yardstick for new-against-old)
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mm-dti_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def bench(env, args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline",
                        "--no-rooflines"] + args, env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"bench.py failed ({r.returncode}): {r.stderr[-600:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["ms_per_step"]


def steps(args):
    for k in range(2):
        for name, env in (("default", {"MMDTI_DETERMINISTIC": "0"}), ("deterministic", {"MMDTI_DETERMINISTIC": "1"})):
            print(f"round {k} {name:14s} {bench(env, args):.3f} ms/step", flush=True)


def ab(old, new, args):
    for k in range(2):
        for name, lib in (("old", old), ("old-again", old), ("new", new)):
            print(f"round {k} {name:10s} {bench({'MMDTI_HIP_LIB': os.path.abspath(lib)}, args):.3f} ms/step", flush=True)


def _time(fn, n=20):
    import torch
    for _ in range(3):
        fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def sites():
    import torch
    from mmdti_hip import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    R = lambda *s: torch.randn(*s, device="cuda", generator=g)
    rows, D = 33280, 512                       # the headline shape's tower-1 token rows
    x, gamma, dy = R(rows, D), R(D), R(rows, D).bfloat16()
    _, _, mean, rstd = ops.layernorm_fwd(x, gamma, R(D), 1e-5)
    dg, db, cs = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    dyw, xw = R(rows, 512).bfloat16(), R(rows, 512).bfloat16()
    dw, dbw = torch.zeros(512, 512, device="cuda"), torch.zeros(512, device="cuda")
    dy50, dw50 = R(8192, 56).bfloat16()[:, :50], torch.zeros(50, 512, device="cuda")
    x8 = R(8192, 512).bfloat16()
    # the fallback and pair-bias forms: 16 molecules x 64 atoms, 961 edge types (gbf), 8192 tokens (embedding), 8 x 70 atoms at ld = 71 (general
    # pair attention)
    Bg, Ng, E, K = 16, 64, 961, 128
    etg = torch.randint(0, E, (Bg, Ng, Ng), device="cuda", generator=g)
    distg = torch.rand(Bg, Ng, Ng, device="cuda", generator=g) * 6.0
    mulg, biasg, meansg, stdsg = R(E) * 0.3 + 1.0, R(E) * 0.3, torch.rand(K, device="cuda", generator=g) * 3, torch.rand(K, device="cuda", generator=g) * 3 + 0.1
    w1g, b1g, w2g = (R(128, K) * 0.1).bfloat16(), R(128) * 0.1, (R(64, 128) * 0.1).bfloat16()
    ging = R(Bg, 64, Ng, Ng)
    gouts = [torch.zeros(n, device="cuda") for n in (128 * K, 128, 64 * 128, 64, E, E, K, K)]
    gouts[0], gouts[2] = gouts[0].view(128, K), gouts[2].view(64, 128)
    dfeat = R(Bg * Ng * Ng, K).bfloat16()
    ids = torch.randint(0, 31, (8192,), device="cuda", generator=g)
    demb, tab = R(8192, 512), torch.zeros(31, 512, device="cuda")
    Bp, Np, Hp, ldp = 8, 70, 64, 71
    qkvp, dOp, sp = R(Bp * Np, 3 * Hp * 8).bfloat16(), R(Bp * Np, Hp * 8).bfloat16(), R(Bp, Hp, Np, ldp)
    gp = torch.zeros(Bp, Hp, Np, ldp, device="cuda")
    cases = {
        "gbf_bias_bwd_full 16 x 64 x 64 pairs, 961 edge types": lambda: ops.gbf_bias_bwd_full(ging, distg, etg, mulg, biasg, meansg, stdsg, w1g, b1g, w2g, Ng, *gouts),
        "gbf_features_bwd 65536 pairs, K = 128, 961 edge types": lambda: ops.gbf_features_bwd(distg.view(-1), etg.view(-1), mulg, biasg, meansg, stdsg, dfeat, *gouts[4:]),
        "embedding_bwd 8192 tokens x 512, 31 rows": lambda: ops.embedding_bwd(ids, demb, tab, 0),
        "pair_attn_bwd general kernel 8 x 64 heads x 70 x 70 (ld = 71)": lambda: ops.pair_attn_bwd(qkvp, sp, dOp, gp, Bp, Np, Hp, ldp, 0.35, True),
        "layernorm_bwd 33280 x 512 (+ bf16 copy + colsum)": lambda: ops.layernorm_bwd(dy, x, gamma, mean, rstd, dg, db, bf16_copy=(0.0, 0, cs)),
        "colsum 33280 x 512": lambda: ops.colsum(dyw, dbw),
        "linear_bwd_weight 512 x 512 over 33280 rows, db": lambda: ops.linear_bwd_weight(dyw, xw, dw, db=dbw),
        "linear_bwd_weight 50 x 512 over 8192 rows (atomic split-K by default)": lambda: ops.linear_bwd_weight(dy50, x8, dw50),
    }
    for name, fn in cases.items():
        ops.set_deterministic(False)
        t0 = _time(fn)
        ops.set_deterministic(True)
        t1 = _time(fn)
        print(f"{name:75s} default {t0:8.1f} us   fixed-order {t1:8.1f} us", flush=True)
    ops.set_deterministic(False)


def scatter():
    import torch
    from oracle import mmdti_oracle as O
    from g9util import load_fixture_weights, product_model, tiny_cfg
    from mmdti_hip import ops
    from mmdti_hip.functional import CELossFn
    from mmdti_hip.runtime import dropout_state
    ocfg = tiny_cfg("classification", 40)
    ocfg.unimol = O.UniMolCfg(layers=2, dim=512, ffn=256, heads=64, K=128, vocab=31)
    ocfg.cross, ocfg.roberta = O.CrossCfg(dim=512, heads=16, ffn=128), O.RobertaCfg(layers=1, dim=512, heads=8, ffn=128, vocab=40, max_pos=140)
    model = product_model(ocfg).cuda().train()
    load_fixture_weights(model, O.init_params(ocfg, seed=12, std=0.05))
    batch, label = O.synth_batch(36, 128, 128, ocfg, seed=4, ragged=False)
    dev = {k: v.cuda() for k, v in batch.items()}

    def step():
        dropout_state.reseed(5)
        model.zero_grad(set_to_none=True)
        logits, infonce, ct = model(**dev, return_infonce_loss=True, return_ct_loss=True, net_target=label.cuda())
        (CELossFn.apply(logits, label.cuda()) + 0.1 * infonce + 0.1 * ct).backward()
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    for mode in (False, True):
        ops.set_deterministic(mode)
        runs = [step() for _ in range(5)]
        worst = {}
        for n in runs[0]:
            ref = runs[0][n]
            d = max(float((r[n] - ref).abs().max()) for r in runs[1:])
            worst[n] = (d, d / (float(ref.abs().max()) + 1e-30))
        moved = {n: v for n, v in worst.items() if v[0] > 0}
        print(f"{'deterministic' if mode else 'default'} mode: {len(moved)} of {len(worst)} parameter gradients differ between five runs", flush=True)
        for n, (d, rel) in sorted(moved.items(), key=lambda t: -t[1][1])[:12]:
            print(f"   {n:60s} max |diff| {d:.3e}   / max |grad| {rel:.3e}")
    ops.set_deterministic(False)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "sites":
        sites()
    elif what == "scatter":
        scatter()
    elif what == "steps":
        steps(sys.argv[2:])
    elif what == "ab":
        ab(sys.argv[2], sys.argv[3], sys.argv[4:])
    else:
        raise SystemExit(__doc__)
