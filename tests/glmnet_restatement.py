"""The reference's ``glfnet`` and ``glfnet_mlp`` (``EEG2Video/models/models.py:105-123, 352-413``) restated with torch functions in
eval mode, from a state dict with the reference's names.  ``dtype=torch.float64`` is what the device and the fixture are compared
with; ``torch.float32`` gives the distance an fp32 implementation may sit from it.

* ``shallownet``: ``Conv2d(1, F, (1, taps))`` -> ``Conv2d(F, F, (C, 1))`` -> ``BatchNorm2d`` on running statistics -> ELU ->
  ``AvgPool2d((1, pool), (1, stride))`` -> flatten (filter-major) -> ``Linear``.  ``shallownet_maps`` stops before the flatten, in the
  reference's UNFOLDED order; ``shallownet_fold`` is the one filter ``[F][C][taps]`` plus a per-filter constant that the two
  convolutions and the BatchNorm amount to (they are linear with nothing between them), in double.
* ``mlpnet``: flatten -> ``Linear`` -> erf GELU -> ``Linear`` -> GELU -> ``Linear``.
* both heads: ``Linear(2 emb, out)`` on ``cat(global, occipital)``; the occipital net sees rows ``first .. first + count - 1``.
"""
import numpy as np
import torch
import torch.nn.functional as F


def _t(v, dtype):
    return (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).to(dtype)


def sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def shallownet_maps(sd, x, dtype=torch.float64, eps=1e-5, pool=51, stride=5):
    """``x`` ``[B, C, T]`` -> the pooled maps ``[B, F, columns]``; ``sd``: ``net.0.*``, ``net.1.*``, ``net.2.*``"""
    x = _t(x, dtype)[:, None]
    y = F.conv2d(x, _t(sd["net.0.weight"], dtype), _t(sd["net.0.bias"], dtype))
    y = F.conv2d(y, _t(sd["net.1.weight"], dtype), _t(sd["net.1.bias"], dtype))
    y = F.batch_norm(y, _t(sd["net.2.running_mean"], dtype), _t(sd["net.2.running_var"], dtype), _t(sd["net.2.weight"], dtype),
                     _t(sd["net.2.bias"], dtype), False, 0.0, eps)
    y = F.avg_pool2d(F.elu(y), (1, pool), (1, stride))
    return y[:, :, 0]


def shallownet_fold(sd, eps=1e-5):
    """``(w [F, C, taps], c [F])`` in float64: ``BN(conv2(conv1(x)))[f][t] = sum_{c, k} w[f][c][k] x[c][t + k] + c[f]``"""
    d = torch.float64
    w1, b1 = _t(sd["net.0.weight"], d)[:, 0, 0], _t(sd["net.0.bias"], d)                 # [G, taps], [G]
    w2, b2 = _t(sd["net.1.weight"], d)[:, :, :, 0], _t(sd["net.1.bias"], d)              # [F, G, C], [F]
    s = _t(sd["net.2.weight"], d) / torch.sqrt(_t(sd["net.2.running_var"], d) + eps)
    shift = _t(sd["net.2.bias"], d) - _t(sd["net.2.running_mean"], d) * s
    w = torch.einsum("fgc,gk->fck", w2, w1)
    c = b2 + torch.einsum("fgc,g->f", w2, b1)
    return w * s[:, None, None], c * s + shift


def shallownet_maps_folded(w, c, x, pool=51, stride=5):
    y = F.conv2d(x.to(w.dtype)[:, None], w[:, None], c)                                   # [B, F, 1, T - taps + 1]
    return F.avg_pool2d(F.elu(y), (1, pool), (1, stride))[:, :, 0]


def shallownet(sd, x, dtype=torch.float64, **kw):
    maps = shallownet_maps(sd, x, dtype, **kw)
    return F.linear(maps.flatten(1), _t(sd["out.weight"], dtype), _t(sd["out.bias"], dtype)), maps


def glfnet(sd, x, dtype=torch.float64, first=50, count=12, **kw):
    """``x`` ``[B, C, T]`` -> dict(logits, features ``[B, 2 emb]``, maps_global, maps_occipital)"""
    x = _t(x, dtype)
    g, mg = shallownet(sub(sd, "globalnet."), x, dtype, **kw)
    o, mo = shallownet(sub(sd, "occipital_localnet."), x[:, first:first + count], dtype, **kw)
    feat = torch.cat((g, o), 1)
    return {"logits": F.linear(feat, _t(sd["out.weight"], dtype), _t(sd["out.bias"], dtype)), "features": feat, "maps_global": mg,
            "maps_occipital": mo}


def mlpnet(sd, x, dtype=torch.float64):
    y = _t(x, dtype).flatten(1)
    y = F.gelu(F.linear(y, _t(sd["net.1.weight"], dtype), _t(sd["net.1.bias"], dtype)))
    y = F.gelu(F.linear(y, _t(sd["net.3.weight"], dtype), _t(sd["net.3.bias"], dtype)))
    return F.linear(y, _t(sd["net.5.weight"], dtype), _t(sd["net.5.bias"], dtype))


def glfnet_mlp(sd, x, dtype=torch.float64, first=50, count=12):
    """``x`` ``[B, C, bands]`` -> dict(logits, features)"""
    x = _t(x, dtype)
    feat = torch.cat((mlpnet(sub(sd, "globalnet."), x, dtype), mlpnet(sub(sd, "occipital_localnet."), x[:, first:first + count], dtype)), 1)
    return {"logits": F.linear(feat, _t(sd["out.weight"], dtype), _t(sd["out.bias"], dtype)), "features": feat}


def rel_err(a, b):
    a, b = _t(a, torch.float64), _t(b, torch.float64)
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))
