"""Plain-torch restatement of ``transformers``' CLIP text transformer (``CLIPTextModel.forward(input_ids)[0]``), for the shapes the
committed fixture does not cover: token + position embeddings, pre-LN encoder layers under the causal (``triu``) mask -- no padding
mask --, ``final_layer_norm``.  ``tests/test_text_host.py`` pins it to ``tests/golden/clip_text_tiny.npz``, which
``tests/golden/make_text_golden.py`` wrote from ``transformers`` itself.

Measured when ``make_text_golden.py`` wrote the committed fixture (max |a-b| / max |b|, fp32 on the CPU against the float64 run of
this restatement; ``transformers`` 5.15.0, torch CPU): on the fixture's own weights and ids this restatement sits 6.3e-7 and
``transformers`` 7.9e-7 from it, and they agree with each other to 5.4e-7; at the full SD-v1-4 size (12 layers, 768 / 12 / 3072, one
seeded draw of weights with the fixture's gains, 2 x 77 ids) 1.3e-6 and 1.2e-6, agreeing to 8.8e-7.  The figures depend on the gains of
the q / k projections (sharper softmax rows give larger distances: 3.6e-6 at the tiny size with gains of 3); these are the ones
every document of the repository quotes.
"""
import torch
import torch.nn.functional as F

from eeg2video_amd.weights import TextConfig


def _act(h, name):
    if name == "quick_gelu":
        return h * torch.sigmoid(1.702 * h)
    if name == "gelu":
        return F.gelu(h)
    raise ValueError(name)


def clip_text_forward(sd, input_ids, cfg: TextConfig, dtype=torch.float32):
    """``sd``: tensors or arrays under the checkpoint's keys (``text_model.`` prefix); ``input_ids`` ``[B,T]`` -> ``[B,T,hidden]``."""
    w = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}
    ids = torch.as_tensor(input_ids).long()
    b, t = ids.shape
    c, heads = cfg.hidden, cfg.heads
    d = c // heads
    p = "text_model."
    x = w[p + "embeddings.token_embedding.weight"][ids] + w[p + "embeddings.position_embedding.weight"][:t][None]
    mask = torch.full((t, t), float("-inf"), dtype=dtype).triu(1)           # query i sees keys 0 .. i
    for i in range(cfg.layers):
        l = f"{p}encoder.layers.{i}."
        lin = lambda n, v: F.linear(v, w[l + n + ".weight"], w[l + n + ".bias"])
        h = F.layer_norm(x, (c,), w[l + "layer_norm1.weight"], w[l + "layer_norm1.bias"], cfg.layer_norm_eps)
        q, k, v = (lin("self_attn." + n, h).view(b, t, heads, d).transpose(1, 2) for n in ("q_proj", "k_proj", "v_proj"))
        a = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5 + mask, dim=-1) @ v
        x = x + lin("self_attn.out_proj", a.transpose(1, 2).reshape(b, t, c))
        h = F.layer_norm(x, (c,), w[l + "layer_norm2.weight"], w[l + "layer_norm2.bias"], cfg.layer_norm_eps)
        x = x + lin("mlp.fc2", _act(lin("mlp.fc1", h), cfg.hidden_act))
    return F.layer_norm(x, (c,), w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"], cfg.layer_norm_eps)


def causal_attention(qkv, b, t, heads, dtype=torch.float64):
    """The op alone: ``qkv`` ``[B*T, 3 * heads * 64]`` (q | k | v) -> ``[B*T, heads * 64]``, head dim 64."""
    c = heads * 64
    q, k, v = (z.to(dtype).view(b, t, heads, 64).transpose(1, 2) for z in qkv.split(c, dim=1))
    mask = torch.full((t, t), float("-inf"), dtype=dtype).triu(1)
    a = torch.softmax(q @ k.transpose(-1, -2) * 0.125 + mask, dim=-1) @ v
    return a.transpose(1, 2).reshape(b * t, c)


def rel_err(a, b):
    """max |a - b| / max |b| (the metric of ``test_semantic_predictor_vs_oracle``)"""
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()
