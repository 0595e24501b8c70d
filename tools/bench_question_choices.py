"""Q questions of 32 tokens about ONE C5-shaped scene (tools/bench_choices.py's: 8 views at 518x518, 8 ViT images of 768x768), each
with 4 choices of 8 tokens: the one pass (G2VLM.score_questions) beside what a caller can do today on a shared scene cache - Q
times the pair (_chat_question, score_continuations) with the cache's length set back in between.  Same process, alternating,
HIP events, --reps repeats after --warmup; the time of one scene prefill is shown beside them.

One und-expert weight pass instead of 2 Q is the expectation; no ratio is demanded.
    python tools/bench_question_choices.py [--qs 1,4,16] [--reps 10] [--warmup 2] [--top-k 0] [--out profiles/question_choices.json]
    python tools/bench_question_choices.py --kernel [--out profiles/topk_kernel.json]
--kernel: g2v_topk_rows_bf16 against g2v_logprob_rows_bf16 on the same logits (rows 32 and 1024, n = 151 936, k = 1, 5, 32).
The per-kernel split of the Q = 16 pass: rocprofv3 --kernel-trace --stats -- python tools/bench_question_choices.py --qs 16 --only pass
                                         python3 tools/rocpd_last_pass.py <results.db> logprob_rows_bf16_kernel
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_questions import HW, NEW_TOKEN_IDS, N_VIEWS, Tok  # noqa: E402

CHOICES, TOKENS = 4, 8
SUFFIX = "<|im_end|>\n<|im_start|>assistant"


def timed_pairs(fns, reps, warmup):
    """ms of each of `reps` calls of every function of `fns`, called in turn (a, b, a, b, ..), after `warmup` rounds."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    evs = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs[i].append((e0, e1))
    torch.cuda.synchronize()
    return [[e0.elapsed_time(e1) for e0, e1 in ev] for ev in evs]


def stats(prefix, ms):
    return {f"{prefix}_ms_median": round(statistics.median(ms), 4), f"{prefix}_ms_min": round(min(ms), 4), f"{prefix}_ms_max": round(max(ms), 4)}


def kernel_bench(a):
    from g2vlm_amd import hip
    out = {"metric": "g2v_topk_rows_bf16 vs g2v_logprob_rows_bf16 on the same bf16 logits, n = 151936", "device": torch.cuda.get_device_name(0),
           "reps": a.reps, "warmup": a.warmup, "cases": []}
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    for rows in (32, 1024):
        x = (torch.randn((rows, 151936), generator=g, device="cuda") * 4).to(torch.bfloat16)
        t = torch.randint(0, 151936, (rows,), generator=g, device="cuda").int()
        lp, lse = (torch.empty(rows, dtype=torch.float32, device="cuda") for _ in range(2))
        rank = torch.empty(rows, dtype=torch.int32, device="cuda")
        fns = [lambda: hip.logprob_rows_bf16(x, t, lse=lse, rank=rank, out=lp)]
        for k in (1, 5, 32):
            idx = torch.empty((rows, k), dtype=torch.int32, device="cuda")
            val = torch.empty((rows, k), dtype=torch.float32, device="cuda")
            fns.append(lambda k=k, idx=idx, val=val: hip.topk_rows_bf16(x, k, out_idx=idx, out_val=val))
        ms = timed_pairs(fns, a.reps, a.warmup)
        case = {"rows": rows, "MB_read": round(rows * 151936 * 2 / 1e6, 1), **stats("logprob", ms[0])}
        for k, m in zip((1, 5, 32), ms[1:]):
            case.update(stats(f"topk_k{k}", m))
        out["cases"].append(case)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qs", default="1,4,16")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--only", choices=("pass",), default=None, help="pass: only the one pass (for a kernel trace)")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    if a.kernel:
        out = kernel_bench(a)
    else:
        import numpy as np
        from PIL import Image
        from g2vlm_amd import host
        from g2vlm_amd.g2vlm_utils import build_model, configs_from_dims
        from g2vlm_amd.synthetic import REAL_DIMS, SyntheticStateDict
        dims, dev = REAL_DIMS, torch.device("cuda", 0)
        model = build_model(*configs_from_dims(dims), SyntheticStateDict(dims, dev, seed=0), dev)
        g = torch.Generator(); g.manual_seed(1000)
        imgs = torch.rand((N_VIEWS, 3, HW, HW), generator=g)
        rng = np.random.default_rng(3000)
        tf = host.QwenVL2ImageTransform(768, 768, 14, device=dev, k_pad=model.weights["vit.patch.w"].shape[1])
        vit_in = []
        for _ in range(N_VIEWS):
            pv, thw = tf([Image.fromarray(rng.integers(0, 256, size=(768, 768, 3), dtype=np.uint8))])
            vit_in.append((pv, tuple(int(v) for v in thw[0])))
        tok = Tok()

        def transform():
            it = iter(vit_in)
            return lambda _im: (lambda pv, thw: (pv, torch.tensor([list(thw)])))(*next(it))

        def scene():
            past, lens, rope = model._chat_geometry(tok, NEW_TOKEN_IDS, None, imgs)
            return model._chat_vit(past, lens, rope, NEW_TOKEN_IDS, transform(), imgs)

        out = {"metric": f"C5 scene: Q questions of 32 tokens x {CHOICES} choices x {TOKENS} tokens, one pass vs Q x (question prefill + "
                         "score_continuations) on the shared scene cache", "device": torch.cuda.get_device_name(0), "reps": a.reps,
               "warmup": a.warmup, "top_k": a.top_k, "cases": []}
        if a.only is None:
            (ms,) = timed_pairs([scene], 3, 1)
            out.update(stats("scene_prefill", ms))
        past, lens, rope = scene()
        plen = past.length
        out["prefix_rows"] = plen
        for Q in (int(v) for v in a.qs.split(",")):
            prompts = [f"question {j}?" for j in range(Q)]
            conts = [[[100 + 40 * j + 10 * c + i for i in range(TOKENS)] for c in range(CHOICES)] for j in range(Q)]
            qs = []
            for p, c in zip(prompts, conts):
                ti, ql, qr = model.prepare_prompts_pure_text(lens, rope, [p + SUFFIX], tok, NEW_TOKEN_IDS)
                qs.append((ti, model.prepare_start_tokens(ql, qr, tok, NEW_TOKEN_IDS), c))
            assert all(q[0]["packed_text_ids"].numel() == 32 for q in qs)

            def one_pass():
                return model.score_questions(past, qs, top_k=a.top_k)

            def today():
                res = []
                for p, c in zip(prompts, conts):
                    _, gi = model._chat_question(past, lens, rope, tok, NEW_TOKEN_IDS, p)
                    res.append(model.score_continuations(past, gi, c, top_k=a.top_k))
                    past.length = plen
                return res
            ms = timed_pairs([one_pass] if a.only else [one_pass, today], a.reps, a.warmup)
            case = {"Q": Q, "rows": Q * (32 + CHOICES * TOKENS), **stats("one_pass", ms[0])}
            if not a.only:
                case.update(stats("per_question", ms[1]))
                case["per_question_over_one_pass"] = round(case["per_question_ms_median"] / case["one_pass_ms_median"], 3)
                x, y = one_pass(), today()
                case["max_abs_logprob_difference"] = max(float((u["logprobs"] - v["logprobs"]).abs().max()) for s, t in zip(x, y)
                                                         for u, v in zip(s, t))
            out["cases"].append(case)
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
