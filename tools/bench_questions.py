"""B questions about ONE C5-shaped scene (8 views at 518x518, 8 ViT images of 768x768): chat_with_recon_batch with the scene
repeated B times (B prefills, B copies of the scene's KV rows) against chat_with_recon_questions (one scene prefill, one
copy, shared-prefix decode attention), alternating between the two in one process.

Per B and path: prefill ms (wall, device-synchronised), decode ms per step (device events over --steps graph-replayed steps
after --warmup), end-to-end questions/s of the public call (--tokens greedy tokens per answer, EOS disabled) and the peak of
torch.cuda.max_memory_allocated above the weights.  One JSON line per (B, path), then a summary line.
    python tools/bench_questions.py [--batches 1,2,4,8,16] [--reps 2] [--out profiles/questions.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NEW_TOKEN_IDS = dict(bos_token_id=1, eos_token_id=-1, start_of_image=3, end_of_image=4)     # no EOS: every answer is --tokens long
N_VIEWS, HW = 8, 518


class Tok:
    """32-id question, 7-id everything else (as bench.py's C5 workload); real tokenizer files are not available offline."""
    eos_token_id = 2

    def encode(self, text, add_special_tokens=False):
        return list(range(11, 11 + 32)) if "?" in text else [11, 12, 13, 14, 15, 16, 17]

    def decode(self, ids):
        return ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--tokens", type=int, default=96, help="greedy tokens per answer in the end-to-end call")
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.warmup + a.steps <= 512

    import numpy as np
    from PIL import Image
    from g2vlm_amd import host
    from g2vlm_amd.g2vlm_utils import build_model, configs_from_dims
    from g2vlm_amd.synthetic import REAL_DIMS, SyntheticStateDict
    dims, dev = REAL_DIMS, torch.device("cuda", 0)
    model = build_model(*configs_from_dims(dims), SyntheticStateDict(dims, dev, seed=0), dev)
    model.use_decode_graph = True
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

    def transform(n_scenes):
        it = iter(vit_in * n_scenes)
        return lambda _im: (lambda pv, thw: (pv, torch.tensor([list(thw)])))(*next(it))

    def sync_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, 1e3 * (time.perf_counter() - t0)

    def step_ms(st):
        for _ in range(a.warmup):
            eng.decode_step_batch(st)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            eng.decode_step_batch(st)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    def run(path, B):
        n_steps = a.warmup + a.steps
        if path == "batch":
            def prefill():
                return [model._chat_prefill(tok, NEW_TOKEN_IDS, transform(1), None, imgs, prompt) for _ in range(B)]
            pairs, pre_ms = sync_ms(prefill)
            st = eng.decode_begin_batch([p for p, _ in pairs], [int(gi["packed_start_tokens"][0]) for _, gi in pairs],
                                        [int(gi["packed_query_position_ids"][0, 0]) for _, gi in pairs], n_steps, use_graph=True)
            plen = pairs[0][0].length
        else:
            (past, qs), pre_ms = sync_ms(lambda: model.prefill_questions(tok, NEW_TOKEN_IDS, transform(1), None, imgs, [prompt] * B))
            st = eng.decode_begin_shared(past, [q for q, _ in qs], [int(gi["packed_start_tokens"][0]) for _, gi in qs],
                                         [int(gi["packed_query_position_ids"][0, 0]) for _, gi in qs], n_steps, use_graph=True)
            plen = past.length
        dec = step_ms(st)
        del st
        pairs = qs = past = None                              # noqa: F841  (free the caches before the end-to-end call)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        if path == "batch":
            _, e2e = sync_ms(lambda: model.chat_with_recon_batch(tok, NEW_TOKEN_IDS, transform(B), None, [(imgs, prompt)] * B, a.tokens))
        else:
            _, e2e = sync_ms(lambda: model.chat_with_recon_questions(tok, NEW_TOKEN_IDS, transform(1), None, imgs, [prompt] * B, a.tokens))
        peak = torch.cuda.max_memory_allocated() - base
        return dict(prefill_ms=pre_ms, decode_ms_per_step=dec, e2e_ms=e2e, questions_per_s=B / (e2e / 1e3), peak_alloc_bytes=peak,
                    prefix_rows=plen)

    batches = [int(b) for b in a.batches.split(",")]
    rows = []
    run("questions", 1)                                      # warm-up: lazy module loads, allocator growth
    for B in batches:
        res = {"batch": [], "questions": []}
        for r in range(a.reps):
            for path in (("batch", "questions") if r % 2 == 0 else ("questions", "batch")):
                res[path].append(run(path, B))
                torch.cuda.empty_cache()
        for path, lst in res.items():
            row = dict(B=B, path=path, reps=len(lst))
            for k in lst[0]:
                row[k] = round(statistics.median(x[k] for x in lst), 3) if k != "peak_alloc_bytes" else max(x[k] for x in lst)
            rows.append(row)
            print(json.dumps(row), flush=True)
    summary = {"metric": "questions about one C5 scene: copied-prefix batch vs shared-prefix decode",
               "tokens_per_answer": a.tokens, "decode_steps_timed": a.steps, "warmup_steps": a.warmup,
               "device": torch.cuda.get_device_name(0), "rows": rows}
    for B in batches:
        b = next(r for r in rows if r["B"] == B and r["path"] == "batch")
        q = next(r for r in rows if r["B"] == B and r["path"] == "questions")
        summary[f"B{B}_decode_step_speedup"] = round(b["decode_ms_per_step"] / q["decode_ms_per_step"], 3)
        summary[f"B{B}_questions_per_s_speedup"] = round(q["questions_per_s"] / b["questions_per_s"], 3)
        summary[f"B{B}_peak_ratio"] = round(b["peak_alloc_bytes"] / max(1, q["peak_alloc_bytes"]), 3)
    print(json.dumps(summary), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
