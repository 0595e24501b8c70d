"""Drop-in counterpart of the reference's inference_chat.py (same flags), running on g2vlm_amd.
--image-path is honoured and an empty --question falls back to the built-in one (H6)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from g2vlm_utils import load_model_and_tokenizer, build_transform, process_conversation  # noqa: E402  (the reference's import line, inference_chat.py:8)

parser = argparse.ArgumentParser()
parser.add_argument("--model-path", type=str, default="InternRobotics/G2VLM-2B-MoT")
parser.add_argument("--image-path", type=str, default="examples/25_0.jpg")
parser.add_argument("--question", type=str, action="append", default=None,
                    help="with --choices it may be given several times: every question is scored over one prefill of the scene")
parser.add_argument("--decode-weights", choices=("bf16", "fp8"), default="bf16",
                    help="fp8: the decode step streams its Linear weights as e4m3 with one power-of-two scale per row")
parser.add_argument("--decode-kv", choices=("bf16", "fp8"), default="bf16",
                    help="fp8: the decode step keeps its KV cache as e4m3 with one power-of-two scale per row and kv head")
parser.add_argument("--choices", nargs="+", default=None, metavar="ANSWER",
                    help="score these candidate answers (log-likelihood, one pass) and print the most likely one instead of generating")
parser.add_argument("--top-k", type=int, default=0, metavar="N",
                    help="with --choices: also print the N most likely first tokens of the answer (at most 32)")


def print_table(choices, scores, details, tokenizer, top_k):
    print(f"{'choice':<24} {'tokens':>6} {'log-prob':>10} {'per token':>10}  first-token rank")
    for text, score, d in zip(choices, scores, details):
        print(f"{text[:24]:<24} {len(d['ids']):>6} {score:>10.4f} {score / len(d['ids']):>10.4f}  {int(d['ranks'][0])}")
    if top_k:                                                # the first position is the same for every choice: the question's own next token
        ids, lps = details[0]["top_ids"][0].tolist(), details[0]["top_logprobs"][0].tolist()
        print("most likely first tokens: " + ", ".join(f"{tokenizer.decode([t])!r} {lp:.3f}" for t, lp in zip(ids, lps)))


def main(argv=None):
    args = parser.parse_args(argv)
    from PIL import Image
    # the reference hands the whole Namespace to the loader (inference_chat.py:18); the loader accepts both forms
    model, tokenizer, new_token_ids, vit_image_transform, dino_transform = load_model_and_tokenizer(args)
    image_transform = build_transform(pixel=768)
    total_params = sum(p.numel() for p in model.parameters()) / 1e9
    print(f"[test] total_params: {total_params}B")
    question = ("If the table (red point) is positioned at 2.6 meters, estimate the depth of the clothes (blue point).  "
                "Calculate or judge based on the 3D center points of these objects. The unit is meter. "
                "Submit your response as one numeric value only.")
    templated = "\n" + question + "\n" + "Please answer the question using a single word or phrase."
    questions = [q for q in (args.question or []) if q]
    if len(questions) > 1 and not args.choices:
        parser.error("several --question need --choices")
    if args.top_k and not args.choices:
        parser.error("--top-k needs --choices")
    if questions:
        templated = questions[0]
    images = [Image.open(args.image_path).convert("RGB")]
    if len(questions) > 1:
        prompts = []
        for q in questions:
            images_q, conversation = process_conversation(images, q)
            prompts.append(conversation)
        results = model.chat_with_recon_questions_choices(tokenizer, new_token_ids, image_transform, dino_transform, images=images_q,
                                                          prompts=prompts, choices=args.choices, top_k=args.top_k)
        for q, (best, scores, details) in zip(questions, results):
            print("question:", q)
            print_table(args.choices, scores, details, tokenizer, args.top_k)
            print("answer: ", args.choices[best])
        return [args.choices[best] for best, _, _ in results]
    images, conversation = process_conversation(images, templated)
    if args.choices:
        best, scores, details = model.chat_with_recon_choices(tokenizer, new_token_ids, image_transform, dino_transform, images=images,
                                                              prompt=conversation, choices=args.choices, top_k=args.top_k)
        print_table(args.choices, scores, details, tokenizer, args.top_k)
        print("answer: ", args.choices[best])
        return args.choices[best]
    response = model.chat_with_recon(tokenizer, new_token_ids, image_transform, dino_transform, images=images,
                                     prompt=conversation, max_length=100)
    print("answer: ", response)
    return response


if __name__ == "__main__":
    main()
