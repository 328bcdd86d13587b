"""Writes ``tests/golden/clip_text_tiny.npz``: the CLIP text encoder fixture, made by ``transformers`` itself.

Run where ``transformers`` is installed (CPU is enough):  ``python tests/golden/make_text_golden.py``

``transformers.CLIPTextModel`` is built at ``TINY_TEXT`` (vocab 128, hidden 128, 2 heads, 2 layers, intermediate 256, 77 positions)
with weights from a seeded torch generator: projection matrices scaled up so that scores and activations have spread (softmax rows
that are far from uniform, GELU inputs on both sides of zero), LayerNorm weights around 1 and biases around 0 with real variation.
Every tensor is rounded to fp16 and stored as fp16 (0.6 MB); the model runs on those values widened to fp32.  The file holds

* the weights under the SD-v1-4 ``text_encoder`` checkpoint's key names (``text_model.`` prefix),
* ``input_ids`` ``[3,77]``: one row bos / tokens / eos-padded as the CLIP tokenizer pads a prompt, two random rows,
* ``out_quick_gelu`` and ``out_gelu`` ``[3,77,128]`` fp32: ``CLIPTextModel(input_ids)[0]`` with ``hidden_act`` set to each,
* ``transformers_version``.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from eeg2video_amd.weights import TINY_TEXT, text_param_spec  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "clip_text_tiny.npz")
BOS, EOS = 126, 127


def make_weights(seed: int = 2024):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in text_param_spec(TINY_TEXT).items():
        leaf = name.rsplit(".", 2)[-2]
        if "layer_norm" in leaf:
            v = torch.randn(shape, generator=g) * 0.25 + (1.0 if name.endswith(".weight") else 0.0)
        elif "embedding" in leaf:
            v = torch.randn(shape, generator=g) * 0.5
        elif name.endswith(".bias"):
            v = torch.randn(shape, generator=g) * 0.1
        else:
            gain = {"q_proj": 1.5, "k_proj": 1.5, "fc1": 1.5}.get(leaf, 1.0)
            v = torch.randn(shape, generator=g) * gain / shape[1] ** 0.5
        sd[name] = v.half()
    return sd


def make_ids(seed: int = 7):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, TINY_TEXT.vocab_size, (3, TINY_TEXT.max_positions), generator=g)
    ids[0, 0] = BOS
    ids[0, 1:12] = torch.randint(0, BOS, (11,), generator=g)
    ids[0, 12:] = EOS
    return ids


def run_transformers(sd, ids, hidden_act):
    """``CLIPTextModel(input_ids)[0]`` in fp32 on the CPU; keys mapped to whatever prefix this ``transformers`` uses."""
    from transformers import CLIPTextConfig, CLIPTextModel
    c = TINY_TEXT
    cfg = CLIPTextConfig(vocab_size=c.vocab_size, hidden_size=c.hidden, intermediate_size=c.intermediate, num_hidden_layers=c.layers,
                         num_attention_heads=c.heads, max_position_embeddings=c.max_positions, hidden_act=hidden_act,
                         layer_norm_eps=c.layer_norm_eps, bos_token_id=BOS, eos_token_id=EOS, pad_token_id=EOS)
    model = CLIPTextModel(cfg).eval()
    own = model.state_dict()
    prefixed = any(k.startswith("text_model.") for k in own)
    load = {(k if prefixed else k[len("text_model."):]): torch.as_tensor(v).float() for k, v in sd.items()}
    missing, unexpected = model.load_state_dict(load, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    with torch.no_grad():
        return model(input_ids=torch.as_tensor(ids).long())[0].float().numpy()


def main():
    import transformers
    sd, ids = make_weights(), make_ids()
    out = {k: v.numpy() for k, v in sd.items()}
    out["input_ids"] = ids.numpy().astype(np.int64)
    out["out_quick_gelu"] = run_transformers(sd, ids, "quick_gelu")
    out["out_gelu"] = run_transformers(sd, ids, "gelu")
    out["transformers_version"] = np.array(transformers.__version__)
    np.savez(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes; transformers", transformers.__version__)


if __name__ == "__main__":
    main()
