"""Ask a model tuned by ``train.py`` a question: Alpaca prompt in, generated tokens out.

    python generate.py --model_dir out --instruction "Name three primary colours." \
        [--input "..."] [--max_new_tokens 64] [--temperature 0.7 --top_p 0.9] [--graph]
        [--weight_format {native,mxfp8,mxfp4}] [--kv_cache_format {mxfp8}]

``--model_dir`` is a directory written by ``train.py`` (config.json + weights + tokenizer). The
prompt is built from the templates the training data used (``smdt_amd.data.sft.PROMPT_DICT``) and
continued with the KV-cache decoder (``HFCausalLM.generate``; greedy unless ``--temperature`` is
given). The new token ids are printed, and the decoded text when the tokenizer can decode: the
offline ``HashWordTokenizer`` hashes words to ids and cannot. ``--weight_format`` (GPU) streams the
layers' weights through the decode GEMM kernel: ``native`` reads the 16-bit parameters, ``mxfp8`` /
``mxfp4`` (bf16 models) a block-scaled copy made once; the LM head stays 16-bit and the 16-bit
parameters stay in memory. ``--kv_cache_format mxfp8`` keeps the K/V cache as MXFP8 (E4M3 elements,
one scale byte per 32: 51.6 % of the 16-bit cache; head dimension 64 or 128).
"""
import argparse
import json
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(_HERE, "..", "..")))

import torch  # noqa: E402

from smdt_amd.data import sft  # noqa: E402
from smdt_amd.models.hf import HFCausalLM  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model_dir", required=True, help="directory written by train.py")
    ap.add_argument("--instruction", required=True)
    ap.add_argument("--input", default="")
    ap.add_argument("--max_new_tokens", type=int, default=64)
    ap.add_argument("--temperature", type=float, default=0.0, help="0: greedy")
    ap.add_argument("--top_p", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--graph", action="store_true", help="capture the decode step in a graph (GPU)")
    ap.add_argument("--weight_format", choices=["native", "mxfp8", "mxfp4"], default=None,
                    help="how the decode steps read the layers' weights (default: the model's own linears)")
    ap.add_argument("--kv_cache_format", choices=["mxfp8"], default=None,
                    help="how the K/V cache is stored (default: the model dtype)")
    ap.add_argument("--draft_model_dir", default=None,
                    help="a smaller model with the same vocabulary: greedy speculative decoding (temperature 0)")
    ap.add_argument("--num_draft_tokens", type=int, default=4, help="tokens the draft proposes per round (1 .. 7)")
    args = ap.parse_args(argv)

    gpu = torch.cuda.is_available()
    device = torch.device("cuda", 0) if gpu else torch.device("cpu")
    model = HFCausalLM.from_pretrained(args.model_dir, params_dtype=torch.bfloat16 if gpu else torch.float32,
                                       device=device).eval()
    tokenizer = sft.load_tokenizer(args.model_dir, model_type=model.hf_config.get("model_type"))
    key = "prompt_input" if args.input else "prompt_no_input"
    prompt = sft.PROMPT_DICT[key].format_map({"instruction": args.instruction, "input": args.input})
    ids = tokenizer(prompt, return_tensors="pt").input_ids.to(device)
    spec, reach = {}, model.cfg.max_position_embeddings
    if args.draft_model_dir:
        draft = HFCausalLM.from_pretrained(args.draft_model_dir, params_dtype=torch.bfloat16 if gpu else torch.float32,
                                           device=device).eval()
        spec = dict(draft_model=draft, num_draft_tokens=args.num_draft_tokens, stats={})
        # rejected drafts touch num_draft_tokens positions beyond the last new token, in both models
        reach = min(reach, draft.cfg.max_position_embeddings) - args.num_draft_tokens
    room = reach - ids.shape[1]
    if room < 1:
        raise SystemExit(f"the prompt ({ids.shape[1]} tokens) leaves no room within max_position_embeddings "
                         f"{reach}")
    new = min(args.max_new_tokens, room)
    eos = tokenizer.eos_token_id
    sample = args.temperature > 0
    gen = torch.Generator(device=device).manual_seed(args.seed) if sample else None
    out = model.generate(ids, max_new_tokens=new, do_sample=sample, temperature=args.temperature if sample else 1.0,
                         top_p=args.top_p, eos_token_id=eos, generator=gen, use_graph=args.graph,
                         weight_format=args.weight_format, kv_cache_format=args.kv_cache_format, **spec)
    tokens = out[0, ids.shape[1]:].tolist()
    if eos is not None and eos in tokens:
        tokens = tokens[: tokens.index(eos) + 1]
    print(json.dumps({"prompt_tokens": int(ids.shape[1]), "new_token_ids": tokens, **spec.get("stats", {})}))
    if hasattr(tokenizer, "decode"):
        print(tokenizer.decode(tokens, skip_special_tokens=True))
    else:
        print(f"[{type(tokenizer).__name__} maps words to ids by hashing and cannot decode them: ids only]")


if __name__ == "__main__":
    main()
