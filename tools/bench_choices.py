"""Scoring 4 candidate answers of 8 tokens on ONE C5-shaped scene (8 views at 518x518, 8 ViT images of 768x768, the question
prefilled) in one teacher-forced pass (Engine.score_rows), beside what walking the same 4 x 8 tokens through the decode costs:
8 graph-replayed steps of generate_text_shared's state at B = 4.  Same process, HIP events, --reps repeats after --warmup.

One und-expert weight pass plus one lm_head read against eight of each is the expectation; no ratio is demanded.
    python tools/bench_choices.py [--reps 20] [--warmup 3] [--only score|decode] [--out profiles/choices.json]
The per-kernel split of the pass: rocprofv3 --kernel-trace --stats -- python tools/bench_choices.py --only score
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("score", "decode"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    from PIL import Image
    from g2vlm_amd import host
    from g2vlm_amd.engine import pack_continuations
    from g2vlm_amd.g2vlm_utils import build_model, configs_from_dims
    from g2vlm_amd.synthetic import REAL_DIMS, SyntheticStateDict
    dims, dev = REAL_DIMS, torch.device("cuda", 0)
    model = build_model(*configs_from_dims(dims), SyntheticStateDict(dims, dev, seed=0), dev)
    eng = model.engine
    g = torch.Generator(); g.manual_seed(1000)
    imgs = torch.rand((N_VIEWS, 3, HW, HW), generator=g)
    rng = np.random.default_rng(3000)
    tf = host.QwenVL2ImageTransform(768, 768, 14, device=dev, k_pad=model.weights["vit.patch.w"].shape[1])
    vit_in = []
    for _ in range(N_VIEWS):
        pv, thw = tf([Image.fromarray(rng.integers(0, 256, size=(768, 768, 3), dtype=np.uint8))])
        vit_in.append((pv, tuple(int(v) for v in thw[0])))
    tok = Tok()
    prompt = "How far is the chair from the door?"

    def transform():
        it = iter(vit_in)
        return lambda _im: (lambda pv, thw: (pv, torch.tensor([list(thw)])))(*next(it))

    def timed(fn):
        """ms of each of --reps calls of fn (HIP events), after --warmup calls."""
        for _ in range(a.warmup):
            fn()
        evs = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in evs]

    out = {"metric": f"C5 scene: {CHOICES} choices x {TOKENS} tokens, one scoring pass vs {TOKENS} shared-prefix decode steps at B = {CHOICES}",
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup}
    if a.only != "decode":
        past, gi = model._chat_prefill(tok, NEW_TOKEN_IDS, transform(), None, imgs, prompt)
        conts = [[100 + 10 * j + i for i in range(TOKENS)] for j in range(CHOICES)]
        ids, poss, seg_lens, targets = pack_continuations(int(gi["packed_start_tokens"][0]), int(gi["packed_query_position_ids"][0, 0]), conts)
        d_ids, d_tg = model._dev_i32(torch.tensor(ids)), model._dev_i32(torch.tensor(targets))
        d_pos = model._dev_i32(torch.tensor(poss).expand(3, -1))
        ms = timed(lambda: eng.score_rows(past, past.length, d_ids, d_pos, seg_lens, d_tg))
        out.update(prefix_rows=past.length, score_pass_ms_median=round(statistics.median(ms), 4), score_pass_ms_min=round(min(ms), 4),
                   score_pass_ms_max=round(max(ms), 4))
        del past
    if a.only != "score":
        n_steps = (a.warmup + a.reps) * TOKENS
        past, qs = model.prefill_questions(tok, NEW_TOKEN_IDS, transform(), None, imgs, [prompt] * CHOICES)
        st = eng.decode_begin_shared(past, [q for q, _ in qs], [int(gi["packed_start_tokens"][0]) for _, gi in qs],
                                     [int(gi["packed_query_position_ids"][0, 0]) for _, gi in qs], n_steps, use_graph=True)

        def steps():
            for _ in range(TOKENS):
                eng.decode_step_batch(st)
        ms = timed(steps)
        out.update(shared_prefix_rows=past.length, decode_8_steps_ms_median=round(statistics.median(ms), 4),
                   decode_8_steps_ms_min=round(min(ms), 4), decode_8_steps_ms_max=round(max(ms), 4))
    if a.only is None:
        out["decode_over_score"] = round(out["decode_8_steps_ms_median"] / out["score_pass_ms_median"], 3)
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
