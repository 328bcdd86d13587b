"""The reference's ``myTransformer.forward`` in eval mode (``EEG2Video_New/Seq2Seq/my_autoregressive_transformer.py:16-192``) restated
with ``torch.nn.functional`` alone, for any ``Seq2SeqConfig`` and any dtype (the tests run it in float64): the yardstick of the device
path where the reference's own module cannot go -- the tiny configs -- and, at the default config, itself checked against the fixture the
reference's module wrote (``tests/golden/seq2seq_ref.npz``).

Like the reference it recomputes every decoder row in every pass (no key / value cache), so that agreement with the device path also
shows that one cached row per pass is the same model.
"""
import math

import torch
import torch.nn.functional as F


def eegnet_features(x, w1, bn1, w2, bn2, w3, w4, bn3, bn_eps=1e-5):
    """``MyEEGNet_embedding`` up to the flatten.  ``x`` ``[N, C, T]``; ``w1`` ``[F1,1,1,64]``, ``w2`` ``[F1 D,1,C,1]``, ``w3``
    ``[F1 D,1,1,16]``, ``w4`` ``[F2,F1 D,1,1]``; ``bn*`` = (weight, bias, running_mean, running_var).  Returns ``[N, F2 * ((T//4)//8)]``."""
    def bn(y, p):
        return F.batch_norm(y, p[2], p[3], p[0], p[1], training=False, eps=bn_eps)
    f1, fd = w1.shape[0], w2.shape[0]
    y = x[:, None]                                                    # [N,1,C,T]
    y = bn(F.conv2d(F.pad(y, (31, 32, 0, 0)), w1), bn1)
    y = F.avg_pool2d(F.elu(bn(F.conv2d(y, w2, groups=f1), bn2)), (1, 4))
    y = F.conv2d(F.conv2d(F.pad(y, (7, 8, 0, 0)), w3, groups=fd), w4)
    y = F.avg_pool2d(F.elu(bn(y, bn3)), (1, 8))
    return y.reshape(y.shape[0], -1)


def attention(q, k, v, heads, mask=None):
    """``nn.MultiheadAttention`` after its projections: ``q`` ``[B,Nq,C]``, ``k``, ``v`` ``[B,Nk,C]``; ``mask`` ``[Nq,Nk]`` additive."""
    b, nq, c = q.shape
    d = c // heads
    split = lambda t: t.reshape(b, t.shape[1], heads, d).transpose(1, 2)
    s = split(q) @ split(k).transpose(-1, -2) / math.sqrt(d)
    if mask is not None:
        s = s + mask
    return (torch.softmax(s, dim=-1) @ split(v)).transpose(1, 2).reshape(b, nq, c)


def _mha(sd, p, x, mem, heads, mask=None):
    c = x.shape[-1]
    w, bias = sd[p + ".in_proj_weight"], sd[p + ".in_proj_bias"]
    q = F.linear(x, w[:c], bias[:c])
    k = F.linear(mem, w[c:2 * c], bias[c:2 * c])
    v = F.linear(mem, w[2 * c:], bias[2 * c:])
    return F.linear(attention(q, k, v, heads, mask), sd[p + ".out_proj.weight"], sd[p + ".out_proj.bias"])


def _ln(sd, p, x, eps):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], eps)


def _ff(sd, p, x):
    return F.linear(F.relu(F.linear(x, sd[p + ".linear1.weight"], sd[p + ".linear1.bias"])), sd[p + ".linear2.weight"], sd[p + ".linear2.bias"])


def seq2seq_forward(sd, cfg, src, pe=None, dtype=torch.float64):
    """``sd``: ``myTransformer`` state dict (tensors or arrays, reference names); ``src`` ``[B, windows, electrodes, samples]``;
    ``pe`` ``[windows, d_model]`` (``None``: rows of ``sd['positional_encoding.pe']``).
    Returns ``dict(enc_out [B,W,C], tokens [B,steps+1,C], txt [B,classes], latents [B,steps+1,c,h,w])``."""
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    src = torch.as_tensor(src).to(dtype)
    b, w = src.shape[:2]
    e = "eeg_embedding."
    bn = lambda n: tuple(sd[f"{e}{n}.{leaf}"] for leaf in ("weight", "bias", "running_mean", "running_var"))
    feats = eegnet_features(src.reshape(b * w, cfg.electrodes, cfg.samples), sd[e + "block_1.1.weight"], bn("block_1.2"),
                            sd[e + "block_2.0.weight"], bn("block_2.1"), sd[e + "block_3.1.weight"], sd[e + "block_3.2.weight"],
                            bn("block_3.3"), cfg.bn_eps)
    x = F.linear(feats, sd[e + "embedding.weight"], sd[e + "embedding.bias"]).reshape(b, w, -1)
    if pe is None:
        pe = sd["positional_encoding.pe"].reshape(-1, cfg.d_model)[:w]
    x = x + torch.as_tensor(pe).to(dtype)[None, :w]
    for i in range(cfg.encoder_layers):
        p = f"transformer_encoder.layers.{i}"
        x = _ln(sd, p + ".norm1", x + _mha(sd, p + ".self_attn", x, x, cfg.heads), cfg.norm_eps)
        x = _ln(sd, p + ".norm2", x + _ff(sd, p, x), cfg.norm_eps)
    enc = x
    tok = torch.zeros(b, 1, cfg.d_model, dtype=dtype)
    for step in range(cfg.steps):
        n = tok.shape[1]
        mask = torch.full((n, n), float("-inf"), dtype=dtype).triu(1)
        y = tok
        for i in range(cfg.decoder_layers):
            p = f"transformer_decoder.layers.{i}"
            y = _ln(sd, p + ".norm1", y + _mha(sd, p + ".self_attn", y, y, cfg.heads, mask), cfg.norm_eps)
            y = _ln(sd, p + ".norm2", y + _mha(sd, p + ".multihead_attn", y, enc, cfg.heads), cfg.norm_eps)
            y = _ln(sd, p + ".norm3", y + _ff(sd, p, y), cfg.norm_eps)
        tok = torch.cat((tok, y[:, -1:]), dim=1)
    txt = F.linear(enc.mean(dim=1), sd["txtpredictor.weight"], sd["txtpredictor.bias"])
    lat = F.linear(tok, sd["predictor.weight"], sd["predictor.bias"]).reshape(b, tok.shape[1], *cfg.latent)
    return {"enc_out": enc, "tokens": tok, "txt": txt, "latents": lat}


def rel_err(a, b):
    """``max|a - b| / max|b|``: the distance every bound of these tests is stated in."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()
