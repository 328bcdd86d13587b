"""State-dict key scheme of the hot path and deterministic synthetic weights.

The hot path has two weight sets, keyed exactly as the reference's checkpoints are:

* ``UNet3DConditionModel`` -- module attribute names of
  ``EEG2Video/models/unet.py:85-207``, ``unet_blocks.py:196-197,269-281,464-470``,
  ``resnet.py:141-172``, ``attention.py:58-87,158-202`` plus the diffusers 0.11.1
  members they instantiate (``to_q/to_k/to_v/to_out.0``, ``ff.net.0.proj``,
  ``ff.net.2``, ``time_embedding.linear_{1,2}``) -- SURVEY.md App. D.
* ``AutoencoderKL`` (diffusers 0.11.1, not in the reference tree).

There are no checkpoints in the container and no network, so every parity test and
the benchmark use weights drawn from a self-contained counter RNG (SplitMix64 keyed
by ``seed`` and an FNV-1a hash of the tensor name).  It is pure integer numpy, so the
GPU box regenerates bit-identical tensors without any torch-version coupling.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Tuple, Union

import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


# --------------------------------------------------------------------------------------
# counter RNG
# --------------------------------------------------------------------------------------
def _fnv1a64(name: str) -> int:
    h = 0xCBF29CE484222325
    for b in name.encode("utf-8"):
        h ^= b
        h = (h * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _splitmix64(x: np.ndarray) -> np.ndarray:
    """One SplitMix64 output per 64-bit counter value (vectorised, wraps mod 2^64)."""
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _stream_base(seed: int, name: str) -> np.uint64:
    s = (int(seed) * 0x9E3779B97F4A7C15 + _fnv1a64(name)) & 0xFFFFFFFFFFFFFFFF
    return _splitmix64(np.array([s], dtype=np.uint64))[0]


def counter_uniform(seed: int, name: str, n: int) -> np.ndarray:
    """``n`` float32 values in [0, 1) with 24 random bits each (exact in float32)."""
    base = _stream_base(seed, name)
    with np.errstate(over="ignore"):
        ctr = base + np.arange(n, dtype=np.uint64)
    bits = _splitmix64(ctr) >> np.uint64(40)
    return (bits.astype(np.float64) * (1.0 / 16777216.0)).astype(np.float32)


def counter_normal(seed: int, name: str, shape: Iterable[int]) -> np.ndarray:
    """Standard normals by Box-Muller over two independent counter streams (float32)."""
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape)) if shape else 1
    u1 = counter_uniform(seed, name + "#u1", n).astype(np.float64)
    u2 = counter_uniform(seed, name + "#u2", n).astype(np.float64)
    u1 = (u1 * 16777216.0 + 1.0) / 16777217.0          # (0, 1): log() is finite
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return z.astype(np.float32).reshape(shape)


# --------------------------------------------------------------------------------------
# configs
# --------------------------------------------------------------------------------------
@dataclass(frozen=True)
class UNetConfig:
    """Mirror of the ctor kwargs of ``UNet3DConditionModel`` that the path uses
    (``EEG2Video/models/unet.py:41-78``); defaults are the SD-v1-4 values."""
    sample_size: int = 64
    in_channels: int = 4
    out_channels: int = 4
    block_out_channels: Tuple[int, ...] = (320, 640, 1280, 1280)
    layers_per_block: int = 2
    cross_attention_dim: int = 768
    attention_head_dim: Union[int, Tuple[int, ...]] = 8   # = NUMBER of heads (unet_blocks.py:257-259); a tuple: per down block (unet.py:110-111)
    norm_num_groups: int = 32
    norm_eps: float = 1e-5
    down_block_types: Tuple[str, ...] = (
        "CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "DownBlock3D")
    up_block_types: Tuple[str, ...] = (
        "UpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D")
    flip_sin_to_cos: bool = True
    freq_shift: int = 0

    @property
    def time_embed_dim(self) -> int:
        return self.block_out_channels[0] * 4


@dataclass(frozen=True)
class VAEConfig:
    """SD-v1-4 ``vae/config.json`` values."""
    in_channels: int = 3
    out_channels: int = 3
    latent_channels: int = 4
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    norm_eps: float = 1e-6
    scaling_factor: float = 0.18215


@dataclass(frozen=True)
class SemanticConfig:
    """Semantic Predictor MLP ``CLIP`` (``EEG2Video/models/train_semantic_predictor.py:11-32``):
    310 -> 10000 -> 10000 -> 10000 -> 10000 -> 77*768 with ReLU between."""
    in_features: int = 310
    hidden: int = 10000
    tokens: int = 77


TINY_SEMANTIC = SemanticConfig(in_features=22, hidden=96, tokens=7)


def semantic_param_spec(cfg: SemanticConfig, cross_attention_dim: int) -> "OrderedDict[str, Tuple[int, ...]]":
    """``nn.Sequential`` keys of the reference module: ``mlp.{0,2,4,6,8}.{weight,bias}``."""
    spec: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    dims = [cfg.in_features, cfg.hidden, cfg.hidden, cfg.hidden, cfg.hidden, cfg.tokens * cross_attention_dim]
    for i in range(5):
        _lin(spec, f"mlp.{2 * i}", dims[i + 1], dims[i])
    return spec


@dataclass(frozen=True)
class TextConfig:
    """``CLIPTextModel`` of the SD checkpoint's ``text_encoder/config.json`` (``transformers`` ``CLIPTextConfig``: ``vocab_size``,
    ``hidden_size``, ``num_attention_heads``, ``num_hidden_layers``, ``intermediate_size``, ``max_position_embeddings``, ``hidden_act``,
    ``layer_norm_eps``); defaults are the SD-v1-4 values.  The head dim is 64 (``hidden == 64 * heads``)."""
    vocab_size: int = 49408
    hidden: int = 768
    heads: int = 12
    layers: int = 12
    intermediate: int = 3072
    max_positions: int = 77
    hidden_act: str = "quick_gelu"
    layer_norm_eps: float = 1e-5


TINY_TEXT = TextConfig(vocab_size=128, hidden=128, heads=2, layers=2, intermediate=256, max_positions=77)

#: ``e2v_config.text_act`` of a ``hidden_act``
TEXT_ACTS = {"quick_gelu": 0, "gelu": 1}


def text_param_spec(cfg: TextConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """name -> shape of the ``CLIPTextModel`` state dict as the SD-v1-4 ``text_encoder`` checkpoint keys it (``text_model.`` prefix,
    no ``position_ids`` buffer); the engine holds them under ``text.``."""
    spec: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    c = cfg.hidden
    spec["text_model.embeddings.token_embedding.weight"] = (cfg.vocab_size, c)
    spec["text_model.embeddings.position_embedding.weight"] = (cfg.max_positions, c)
    for i in range(cfg.layers):
        p = f"text_model.encoder.layers.{i}"
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            _lin(spec, f"{p}.self_attn.{n}", c, c)
        _norm(spec, f"{p}.layer_norm1", c)
        _norm(spec, f"{p}.layer_norm2", c)
        _lin(spec, f"{p}.mlp.fc1", cfg.intermediate, c)
        _lin(spec, f"{p}.mlp.fc2", c, cfg.intermediate)
    _norm(spec, "text_model.final_layer_norm", c)
    return spec


@dataclass(frozen=True)
class ImageConfig:
    """``ViTForImageClassification`` (``transformers`` ``ViTConfig``: ``hidden_size``, ``num_attention_heads``, ``num_hidden_layers``,
    ``intermediate_size``, ``image_size``, ``patch_size``, the number of labels, ``layer_norm_eps``) with its ``ViTImageProcessor``
    (``preprocessor_config.json``: ``rescale_factor``, ``image_mean``, ``image_std``; the resize is Pillow's BILINEAR to
    ``image_size`` x ``image_size``); defaults are ``google/vit-base-patch16-224``, the classifier of the reference's
    ``img_classify_metric``.  The head dim is 64 (``hidden == 64 * heads``), the activation the erf GELU."""
    hidden: int = 768
    heads: int = 12
    layers: int = 12
    intermediate: int = 3072
    image_size: int = 224
    patch_size: int = 16
    num_labels: int = 1000
    layer_norm_eps: float = 1e-12
    rescale_factor: float = 1 / 255
    image_mean: Tuple[float, float, float] = (0.5, 0.5, 0.5)
    image_std: Tuple[float, float, float] = (0.5, 0.5, 0.5)

    @property
    def tokens(self) -> int:
        return (self.image_size // self.patch_size) ** 2 + 1


#: 197 tokens -- the production count -- for a few hundred thousand parameters (tests/golden/vit_tiny.npz)
TINY_IMAGE = ImageConfig(hidden=128, heads=2, layers=2, intermediate=256, image_size=112, patch_size=8, num_labels=50)


def image_param_spec(cfg: ImageConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """name -> shape of the ``ViTForImageClassification`` state dict as the ``google/vit-base-patch16-224`` checkpoint keys it; the
    engine holds them under ``image.``."""
    spec: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    c = cfg.hidden
    spec["vit.embeddings.cls_token"] = (1, 1, c)
    spec["vit.embeddings.position_embeddings"] = (1, cfg.tokens, c)
    _conv(spec, "vit.embeddings.patch_embeddings.projection", c, 3, cfg.patch_size)
    for i in range(cfg.layers):
        p = f"vit.encoder.layer.{i}"
        for n in ("query", "key", "value"):
            _lin(spec, f"{p}.attention.attention.{n}", c, c)
        _lin(spec, f"{p}.attention.output.dense", c, c)
        _lin(spec, f"{p}.intermediate.dense", cfg.intermediate, c)
        _lin(spec, f"{p}.output.dense", c, cfg.intermediate)
        _norm(spec, f"{p}.layernorm_before", c)
        _norm(spec, f"{p}.layernorm_after", c)
    _norm(spec, "vit.layernorm", c)
    _lin(spec, "classifier", cfg.num_labels, c)
    return spec


@dataclass(frozen=True)
class ClipVisionConfig:
    """``CLIPVisionModelWithProjection`` (``transformers`` ``CLIPVisionConfig``: ``hidden_size``, ``num_attention_heads``,
    ``num_hidden_layers``, ``intermediate_size``, ``image_size``, ``patch_size``, ``projection_dim``, ``hidden_act``,
    ``layer_norm_eps``) with its ``CLIPImageProcessor`` (``preprocessor_config.json``: ``size.shortest_edge`` = ``resize_edge``,
    ``resample`` in Pillow's codes, a centre crop of ``image_size``, ``rescale_factor``, ``image_mean``, ``image_std``); defaults are
    ``openai/clip-vit-base-patch32``, the model of the reference's ``clip_score``.  The head dim is 64 (``hidden == 64 * heads``)."""
    hidden: int = 768
    heads: int = 12
    layers: int = 12
    intermediate: int = 3072
    image_size: int = 224
    patch_size: int = 32
    projection_dim: int = 512
    hidden_act: str = "quick_gelu"
    layer_norm_eps: float = 1e-5
    resize_edge: int = 224
    resample: int = 3
    rescale_factor: float = 1 / 255
    image_mean: Tuple[float, float, float] = (0.48145466, 0.4578275, 0.40821073)
    image_std: Tuple[float, float, float] = (0.26862954, 0.26130258, 0.27577711)

    @property
    def tokens(self) -> int:
        return (self.image_size // self.patch_size) ** 2 + 1


#: 50 tokens -- B/32's count -- for a few hundred thousand parameters (tests/golden/clip_vision_tiny.npz)
TINY_CLIP_VISION = ClipVisionConfig(hidden=128, heads=2, layers=2, intermediate=256, image_size=112, patch_size=16, projection_dim=64,
                                    resize_edge=112)


def clip_vision_param_spec(cfg: ClipVisionConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """name -> shape of the ``CLIPVisionModelWithProjection`` state dict as the ``openai/clip-vit-base-patch32`` checkpoint keys it
    (``pre_layrnorm`` is the checkpoint's spelling; no ``position_ids`` buffer); the engine holds them under ``clipv.``."""
    spec: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    c = cfg.hidden
    spec["vision_model.embeddings.class_embedding"] = (c,)
    spec["vision_model.embeddings.patch_embedding.weight"] = (c, 3, cfg.patch_size, cfg.patch_size)
    spec["vision_model.embeddings.position_embedding.weight"] = (cfg.tokens, c)
    _norm(spec, "vision_model.pre_layrnorm", c)
    for i in range(cfg.layers):
        p = f"vision_model.encoder.layers.{i}"
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            _lin(spec, f"{p}.self_attn.{n}", c, c)
        _norm(spec, f"{p}.layer_norm1", c)
        _norm(spec, f"{p}.layer_norm2", c)
        _lin(spec, f"{p}.mlp.fc1", cfg.intermediate, c)
        _lin(spec, f"{p}.mlp.fc2", c, cfg.intermediate)
    _norm(spec, "vision_model.post_layernorm", c)
    spec["visual_projection.weight"] = (cfg.projection_dim, c)
    return spec


@dataclass(frozen=True)
class Seq2SeqConfig:
    """The reference's ``myTransformer`` (``EEG2Video_New/Seq2Seq/my_autoregressive_transformer.py:123-149``): an EEGNet embedding
    (``electrodes`` x ``samples`` per window, ``F1`` / ``D`` / ``F2``) of each of ``windows`` EEG windows, a post-LN transformer
    encoder and an autoregressive post-LN decoder (``d_model``, ``heads``, ``ffn``, ``encoder_layers`` / ``decoder_layers``; ``steps``
    decoder passes give ``steps + 1`` tokens), a latent predictor (``latent`` = (C, h, w)) and a text-class predictor.  Defaults are
    the values the reference hard-codes."""
    electrodes: int = 62
    samples: int = 100
    windows: int = 7
    F1: int = 16
    D: int = 4
    F2: int = 16
    d_model: int = 512
    heads: int = 4
    ffn: int = 2048
    encoder_layers: int = 2
    decoder_layers: int = 4
    steps: int = 6
    latent: Tuple[int, int, int] = (4, 36, 64)
    txt_classes: int = 13
    norm_eps: float = 1e-5
    bn_eps: float = 1e-5
    num_embeddings: int = 10            # the unused nn.Embedding
    pe_max_len: int = 5000              # rows of the positional buffer in a checkpoint

    @property
    def features(self) -> int:
        """Width of the flattened EEGNet output (the reference's 48)."""
        return self.F2 * ((self.samples // 4) // 8)

    @property
    def latent_size(self) -> int:
        return self.latent[0] * self.latent[1] * self.latent[2]


#: three windows of 5 x 40 and three decoder passes for a few tens of thousands of parameters
TINY_SEQ2SEQ = Seq2SeqConfig(electrodes=5, samples=40, windows=3, d_model=64, heads=4, ffn=128, encoder_layers=1, decoder_layers=2,
                             steps=3, latent=(4, 4, 6))

#: the position table as the engine holds it (``[windows][d_model]``; a checkpoint has ``[1][pe_max_len][d_model]`` under the same name)
SEQ2SEQ_PE_KEY = "positional_encoding.pe"


def seq2seq_unused_key(name: str) -> bool:
    """State-dict entries of ``myTransformer`` its inference never reads: the engine does not hold them."""
    return name == "embedding.weight" or name.startswith("img_embedding.") or name.endswith(".num_batches_tracked")


def seq2seq_param_spec(cfg: Seq2SeqConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """name -> shape of ``myTransformer().state_dict()`` in its order (125 entries at the default config), buffers included:
    the BatchNorm statistics, ``num_batches_tracked`` (shape ``()``) and ``positional_encoding.pe`` ``[1, pe_max_len, d_model]``."""
    spec: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    c, fd = cfg.d_model, cfg.F1 * cfg.D

    def bn(name, n):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            spec[f"{name}.{leaf}"] = (n,)
        spec[f"{name}.num_batches_tracked"] = ()

    def mha(name):
        spec[f"{name}.in_proj_weight"] = (3 * c, c)
        spec[f"{name}.in_proj_bias"] = (3 * c,)
        _lin(spec, f"{name}.out_proj", c, c)

    spec["embedding.weight"] = (cfg.num_embeddings, c)
    _lin(spec, "img_embedding", c, cfg.latent_size)
    e = "eeg_embedding"
    spec[f"{e}.block_1.1.weight"] = (cfg.F1, 1, 1, 64)
    bn(f"{e}.block_1.2", cfg.F1)
    spec[f"{e}.block_2.0.weight"] = (fd, 1, cfg.electrodes, 1)
    bn(f"{e}.block_2.1", fd)
    spec[f"{e}.block_3.1.weight"] = (fd, 1, 1, 16)
    spec[f"{e}.block_3.2.weight"] = (cfg.F2, fd, 1, 1)
    bn(f"{e}.block_3.3", cfg.F2)
    _lin(spec, f"{e}.embedding", c, cfg.features)
    for i in range(cfg.encoder_layers):
        p = f"transformer_encoder.layers.{i}"
        mha(f"{p}.self_attn")
        _lin(spec, f"{p}.linear1", cfg.ffn, c)
        _lin(spec, f"{p}.linear2", c, cfg.ffn)
        _norm(spec, f"{p}.norm1", c)
        _norm(spec, f"{p}.norm2", c)
    for i in range(cfg.decoder_layers):
        p = f"transformer_decoder.layers.{i}"
        mha(f"{p}.self_attn")
        mha(f"{p}.multihead_attn")
        _lin(spec, f"{p}.linear1", cfg.ffn, c)
        _lin(spec, f"{p}.linear2", c, cfg.ffn)
        _norm(spec, f"{p}.norm1", c)
        _norm(spec, f"{p}.norm2", c)
        _norm(spec, f"{p}.norm3", c)
    spec[SEQ2SEQ_PE_KEY] = (1, cfg.pe_max_len, c)
    _lin(spec, "txtpredictor", cfg.txt_classes, c)
    _lin(spec, "predictor", cfg.latent_size, c)
    return spec


def seq2seq_engine_spec(cfg: Seq2SeqConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """What the engine expects under ``s2s.``: ``seq2seq_param_spec`` without the unused entries, the position table as the
    ``[windows, d_model]`` rows that are read."""
    spec: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    for k, shape in seq2seq_param_spec(cfg).items():
        if not seq2seq_unused_key(k):
            spec[k] = (cfg.windows, cfg.d_model) if k == SEQ2SEQ_PE_KEY else shape
    return spec


def seq2seq_position_table(rows: int, d_model: int):
    """The first ``rows`` rows of ``PositionalEncoding.pe`` (``my_autoregressive_transformer.py:97-107``) with the reference's own
    fp32 torch expression, ``[rows, d_model]``."""
    import torch
    pe = torch.zeros(rows, d_model)
    position = torch.arange(0, rows).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2) * -(math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


@dataclass(frozen=True)
class GLMNetConfig:
    """The reference's GLMNet pair (``EEG2Video/models/models.py:105-123, 352-413``): ``glfnet(raw_out, emb, electrodes, samples)`` over
    raw EEG -- a global ``shallownet`` over all electrodes and one over the occipital electrodes ``occ_first .. occ_first + occ_count -
    1``, each ``filters`` temporal filters of ``taps`` taps, a spatial mix, BatchNorm, ELU and an average pool ``pool`` / ``pool_stride``
    -- and ``glfnet_mlp(mlp_out, emb, electrodes * bands)`` over DE features, two ``mlpnet`` (``hidden`` = (512, 256)).  ``raw_out`` /
    ``mlp_out`` 0: that model is absent.  Defaults are the values the reference hard-codes and the sizes its scripts construct."""
    electrodes: int = 62
    samples: int = 200
    occ_first: int = 50
    occ_count: int = 12
    filters: int = 40
    taps: int = 25
    pool: int = 51
    pool_stride: int = 5
    bands: int = 5
    hidden: Tuple[int, int] = (512, 256)
    emb: int = 64
    raw_out: int = 2
    mlp_out: int = 40
    bn_eps: float = 1e-5

    @property
    def pooled_columns(self) -> int:
        """Columns the pool leaves of ``samples - taps + 1`` (the reference's 26; 0 where the row is too short)."""
        t = self.samples - self.taps + 1
        return (t - self.pool) // self.pool_stride + 1 if t >= self.pool else 0

    @property
    def raw_features(self) -> int:
        """Width of a ``shallownet``'s flattened maps (the reference's 1040)."""
        return self.filters * self.pooled_columns


#: 5 electrodes (occipital 2..4) of 40 samples, 8 filters of 5 taps, pool 7 / 3: ten pooled columns
TINY_GLMNET = GLMNetConfig(electrodes=5, samples=40, occ_first=2, occ_count=3, filters=8, taps=5, pool=7, pool_stride=3, hidden=(32, 16),
                           emb=8, raw_out=2, mlp_out=6)


def glmnet_param_spec(cfg: GLMNetConfig, model: str) -> "OrderedDict[str, Tuple[int, ...]]":
    """name -> shape of ``glfnet(...).state_dict()`` (``model="raw"``, 24 entries) or ``glfnet_mlp(...).state_dict()`` (``"mlp"``, 14) in
    the module's order, ``num_batches_tracked`` (shape ``()``) included."""
    spec: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    if model == "raw":
        f = cfg.filters
        for name, c in (("globalnet", cfg.electrodes), ("occipital_localnet", cfg.occ_count)):
            spec[f"{name}.net.0.weight"] = (f, 1, 1, cfg.taps)
            spec[f"{name}.net.0.bias"] = (f,)
            spec[f"{name}.net.1.weight"] = (f, f, c, 1)
            spec[f"{name}.net.1.bias"] = (f,)
            for leaf in ("weight", "bias", "running_mean", "running_var"):
                spec[f"{name}.net.2.{leaf}"] = (f,)
            spec[f"{name}.net.2.num_batches_tracked"] = ()
            _lin(spec, f"{name}.out", cfg.emb, cfg.raw_features)
        _lin(spec, "out", cfg.raw_out, 2 * cfg.emb)
    elif model == "mlp":
        for name, c in (("globalnet", cfg.electrodes), ("occipital_localnet", cfg.occ_count)):
            _lin(spec, f"{name}.net.1", cfg.hidden[0], c * cfg.bands)
            _lin(spec, f"{name}.net.3", cfg.hidden[1], cfg.hidden[0])
            _lin(spec, f"{name}.net.5", cfg.emb, cfg.hidden[1])
        _lin(spec, "out", cfg.mlp_out, 2 * cfg.emb)
    else:
        raise ValueError(f"model {model!r}: 'raw' (glfnet) or 'mlp' (glfnet_mlp)")
    return spec


def glmnet_synth_state_dict(cfg: GLMNetConfig, model: str, seed: int = 42) -> "OrderedDict[str, np.ndarray]":
    """``synth_state_dict(..., mode="perturbed")`` of one model with BatchNorm statistics that show: gamma in 0.75 .. 1.25 (the generic
    draw for a name ``net.2.weight`` would straddle zero), running_mean within +-0.16, running_var 0.5 .. 1.5, ``num_batches_tracked``
    an int64 zero as torch keeps it."""
    sd = synth_state_dict(glmnet_param_spec(cfg, model), seed=seed, mode="perturbed")
    for k in sd:
        if k.endswith("net.2.weight"):
            sd[k] = (0.75 + 0.5 * counter_uniform(seed, k, sd[k].size)).astype(np.float32)
        if k.endswith("num_batches_tracked"):
            sd[k] = np.zeros((), np.int64)
    return sd


#: how ``transformers`` 5 spells the per-layer tensors of the same model (``vit.layers.{i}.`` instead of ``vit.encoder.layer.{i}.``)
_VIT_V5_NAMES = (("attention.q_proj.", "attention.attention.query."), ("attention.k_proj.", "attention.attention.key."),
                 ("attention.v_proj.", "attention.attention.value."), ("attention.o_proj.", "attention.output.dense."),
                 ("mlp.fc1.", "intermediate.dense."), ("mlp.fc2.", "output.dense."))


def image_checkpoint_key(name: str) -> str:
    """A ``ViTForImageClassification`` state-dict name in either spelling -> the checkpoint's (``image_param_spec``)."""
    if name.startswith("vit.layers."):
        rest = name[len("vit.layers."):]
        for new, old in _VIT_V5_NAMES:
            if new in rest:
                rest = rest.replace(new, old)
                break
        return "vit.encoder.layer." + rest
    return name


@dataclass(frozen=True)
class VideoConfig:
    """``VideoMAEForVideoClassification`` (``transformers`` ``VideoMAEConfig``: ``hidden_size``, ``num_attention_heads``,
    ``num_hidden_layers``, ``intermediate_size``, ``image_size``, ``patch_size``, ``tubelet_size``, ``num_frames``, the number of
    labels, ``layer_norm_eps``; ``use_mean_pooling``, erf GELU, biased q / k / v as ``transformers`` 5 builds them) with its
    ``VideoMAEImageProcessor`` (``preprocessor_config.json``: ``size.shortest_edge`` = ``resize_edge``, a centre crop of
    ``image_size``, ``rescale_factor``, ``image_mean``, ``image_std``).  The defaults are ``MCG-NJU/videomae-base-finetuned-kinetics``
    as the reference's ``video_classify_metric`` loads it: ``num_frames=6``.  The head dim is 64."""
    hidden: int = 768
    heads: int = 12
    layers: int = 12
    intermediate: int = 3072
    image_size: int = 224
    patch_size: int = 16
    tubelet_size: int = 2
    num_frames: int = 6
    num_labels: int = 400
    layer_norm_eps: float = 1e-12
    resize_edge: int = 224
    rescale_factor: float = 1 / 255
    image_mean: Tuple[float, float, float] = (0.485, 0.456, 0.406)
    image_std: Tuple[float, float, float] = (0.229, 0.224, 0.225)

    @property
    def tokens(self) -> int:
        return (self.num_frames // self.tubelet_size) * (self.image_size // self.patch_size) ** 2


#: 147 tokens: 4.6 key tiles of 32, 2.3 of 64, 1.15 query blocks of 128 -- every ragged edge of the attention kernel
#: (tests/golden/videomae_tiny.npz)
TINY_VIDEO = VideoConfig(hidden=128, heads=2, layers=2, intermediate=256, image_size=56, patch_size=8, tubelet_size=2, num_frames=6,
                         resize_edge=56, num_labels=50)

#: the one key of the video part that no checkpoint holds: the fixed position table, a buffer ``transformers`` builds at construction
VIDEO_POSITION_KEY = "videomae.embeddings.position_embeddings"


def video_param_spec(cfg: VideoConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """name -> shape of the video part as the engine holds it under ``video.``: ``VideoMAEForVideoClassification.state_dict()`` of
    the installed ``transformers`` -- with the ``Conv3d`` weight ``[C,3,ts,P,P]`` as ``[C,3*ts,P,P]`` (``video_engine_shape``: the
    library's key shapes have at most four axes; a reshape, the bytes are the same) -- plus ``VIDEO_POSITION_KEY`` ``[T,C]``."""
    spec: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    c = cfg.hidden
    spec[VIDEO_POSITION_KEY] = (cfg.tokens, c)
    _conv(spec, "videomae.embeddings.patch_embeddings.projection", c, 3 * cfg.tubelet_size, cfg.patch_size)
    for i in range(cfg.layers):
        p = f"videomae.encoder.layer.{i}"
        for n in ("query", "key", "value"):
            _lin(spec, f"{p}.attention.attention.{n}", c, c)
        _lin(spec, f"{p}.attention.output.dense", c, c)
        _lin(spec, f"{p}.intermediate.dense", cfg.intermediate, c)
        _lin(spec, f"{p}.output.dense", c, cfg.intermediate)
        _norm(spec, f"{p}.layernorm_before", c)
        _norm(spec, f"{p}.layernorm_after", c)
    _norm(spec, "fc_norm", c)
    _lin(spec, "classifier", cfg.num_labels, c)
    return spec


def video_engine_shape(shape) -> Tuple[int, ...]:
    """A tensor shape of ``transformers``' state dict -> the engine's: the 5-D ``Conv3d`` weight with axes 1 and 2 merged."""
    shape = tuple(int(d) for d in shape)
    return (shape[0], shape[1] * shape[2]) + shape[3:] if len(shape) == 5 else shape


def video_checkpoint_spec(cfg: VideoConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """name -> shape of ``VideoMAEForVideoClassification.state_dict()`` itself: ``video_param_spec`` without the position table and
    with the ``Conv3d`` weight in its own five axes."""
    spec = video_param_spec(cfg)
    del spec[VIDEO_POSITION_KEY]
    k = "videomae.embeddings.patch_embeddings.projection.weight"
    spec[k] = (cfg.hidden, 3, cfg.tubelet_size, cfg.patch_size, cfg.patch_size)
    return spec


def video_position_table(n_position: int, d_hid: int):
    """``transformers.models.videomae.modeling_videomae.get_sinusoid_encoding_table``, its numpy formula line by line (float64
    ``np.power`` / ``np.sin`` / ``np.cos``, rounded to fp32 once at the end as ``torch.FloatTensor`` does), so that the table holds
    ``transformers``' own bits and not another libm's -> fp32 ``[n_position, d_hid]``."""
    def get_position_angle_vec(position):
        return [position / np.power(10000, 2 * (hid_j // 2) / d_hid) for hid_j in range(d_hid)]

    table = np.array([get_position_angle_vec(pos_i) for pos_i in range(n_position)])
    table[:, 0::2] = np.sin(table[:, 0::2])
    table[:, 1::2] = np.cos(table[:, 1::2])
    return table.astype(np.float32)


def video_checkpoint_key(name: str) -> str:
    """A ``VideoMAEForVideoClassification`` tensor name in the ORIGINAL checkpoint's spelling (the hub file: bias-free query / key /
    value projections and ``...attention.attention.q_bias`` / ``v_bias`` beside them) or in the installed ``transformers``' -> the
    installed one's (``video_checkpoint_spec``): ``q_bias`` is ``query.bias``, ``v_bias`` is ``value.bias``.  The key projection has no
    bias there; ``video_checkpoint_rename`` supplies zeros."""
    for old, new in ((".attention.attention.q_bias", ".attention.attention.query.bias"),
                     (".attention.attention.v_bias", ".attention.attention.value.bias")):
        if name.endswith(old):
            return name[:-len(old)] + new
    return name


def video_checkpoint_rename(state_dict):
    """A state dict in either spelling -> the installed spelling, with a zero ``key.bias`` wherever the original spelling has none.
    (``transformers`` 5.15 itself has no rename for the original spelling: ``from_pretrained`` reports ``q_bias`` / ``v_bias`` as
    unexpected and initialises the three biases afresh, which drops trained values; that is not followed here.  ``transformers`` 4
    added ``q_bias`` and ``v_bias`` to the query and value projections and no bias to the key projection, which is this mapping.)"""
    out = OrderedDict((video_checkpoint_key(k), v) for k, v in state_dict.items())
    for k in list(out):
        if k.endswith(".attention.attention.key.weight"):
            b = k[:-len("weight")] + "bias"
            if b not in out:
                w = out[k]
                out[b] = w.new_zeros(w.shape[0]) if hasattr(w, "new_zeros") else np.zeros(w.shape[0], dtype=np.asarray(w).dtype)
    return out


#: tiny configs used by the parity tests (oracle finishes in well under a second).
TINY_UNET = UNetConfig(sample_size=8, block_out_channels=(64, 128, 256, 256), cross_attention_dim=64)
TINY_VAE = VAEConfig(block_out_channels=(32, 64, 64, 64), norm_num_groups=8)


# --------------------------------------------------------------------------------------
# key / shape specs
# --------------------------------------------------------------------------------------
def _conv(spec, name, cout, cin, k):
    spec[name + ".weight"] = (cout, cin, k, k)
    spec[name + ".bias"] = (cout,)


def _lin(spec, name, cout, cin, bias=True):
    spec[name + ".weight"] = (cout, cin)
    if bias:
        spec[name + ".bias"] = (cout,)


def _norm(spec, name, c):
    spec[name + ".weight"] = (c,)
    spec[name + ".bias"] = (c,)


def _resnet3d(spec, p, cin, cout, temb):
    # resnet.py:141-172
    _norm(spec, p + ".norm1", cin)
    _conv(spec, p + ".conv1", cout, cin, 3)
    _lin(spec, p + ".time_emb_proj", cout, temb)
    _norm(spec, p + ".norm2", cout)
    _conv(spec, p + ".conv2", cout, cout, 3)
    if cin != cout:
        _conv(spec, p + ".conv_shortcut", cout, cin, 1)


def _transformer3d(spec, p, c, cross):
    # attention.py:58-87 (norm, proj_in, proj_out) and :158-202 (block members)
    _norm(spec, p + ".norm", c)
    _conv(spec, p + ".proj_in", c, c, 1)
    b = p + ".transformer_blocks.0"
    for a, kv in (("attn1", c), ("attn2", cross), ("attn_temp", c)):
        _lin(spec, f"{b}.{a}.to_q", c, c, bias=False)
        _lin(spec, f"{b}.{a}.to_k", c, kv, bias=False)
        _lin(spec, f"{b}.{a}.to_v", c, kv, bias=False)
        _lin(spec, f"{b}.{a}.to_out.0", c, c)
    for n in ("norm1", "norm2", "norm3", "norm_temp"):
        _norm(spec, f"{b}.{n}", c)
    _lin(spec, f"{b}.ff.net.0.proj", 8 * c, c)
    _lin(spec, f"{b}.ff.net.2", c, 4 * c)
    _conv(spec, p + ".proj_out", c, c, 1)


def unet_param_spec(cfg: UNetConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """name -> shape for every tensor of the reference UNet state dict (App. D)."""
    spec: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    boc = cfg.block_out_channels
    temb = cfg.time_embed_dim
    _conv(spec, "conv_in", boc[0], cfg.in_channels, 3)                  # unet.py:85
    _lin(spec, "time_embedding.linear_1", temb, boc[0])                 # unet.py:91
    _lin(spec, "time_embedding.linear_2", temb, temb)
    out_c = boc[0]
    for i, typ in enumerate(cfg.down_block_types):                      # unet.py:113-139
        in_c, out_c = out_c, boc[i]
        for j in range(cfg.layers_per_block):
            _resnet3d(spec, f"down_blocks.{i}.resnets.{j}", in_c if j == 0 else out_c, out_c, temb)
            if typ == "CrossAttnDownBlock3D":
                _transformer3d(spec, f"down_blocks.{i}.attentions.{j}", out_c, cfg.cross_attention_dim)
        if i != len(boc) - 1:
            _conv(spec, f"down_blocks.{i}.downsamplers.0.conv", out_c, out_c, 3)
    mid = boc[-1]                                                       # unet.py:142-156
    _resnet3d(spec, "mid_block.resnets.0", mid, mid, temb)
    _transformer3d(spec, "mid_block.attentions.0", mid, cfg.cross_attention_dim)
    _resnet3d(spec, "mid_block.resnets.1", mid, mid, temb)
    rev = list(reversed(boc))                                           # unet.py:164-202
    out_c = rev[0]
    for i, typ in enumerate(cfg.up_block_types):
        prev = out_c
        out_c = rev[i]
        in_c = rev[min(i + 1, len(boc) - 1)]
        n_layers = cfg.layers_per_block + 1
        for j in range(n_layers):
            skip = in_c if j == n_layers - 1 else out_c                 # unet_blocks.py:431-432
            rin = prev if j == 0 else out_c
            _resnet3d(spec, f"up_blocks.{i}.resnets.{j}", rin + skip, out_c, temb)
            if typ == "CrossAttnUpBlock3D":
                _transformer3d(spec, f"up_blocks.{i}.attentions.{j}", out_c, cfg.cross_attention_dim)
        if i != len(boc) - 1:
            _conv(spec, f"up_blocks.{i}.upsamplers.0.conv", out_c, out_c, 3)
    _norm(spec, "conv_norm_out", boc[0])                                # unet.py:205-207
    _conv(spec, "conv_out", cfg.out_channels, boc[0], 3)
    return spec


def _resnet2d(spec, p, cin, cout):
    _norm(spec, p + ".norm1", cin)
    _conv(spec, p + ".conv1", cout, cin, 3)
    _norm(spec, p + ".norm2", cout)
    _conv(spec, p + ".conv2", cout, cout, 3)
    if cin != cout:
        _conv(spec, p + ".conv_shortcut", cout, cin, 1)


def _vae_mid(spec, p, c):
    _resnet2d(spec, p + ".resnets.0", c, c)
    a = p + ".attentions.0"
    _norm(spec, a + ".group_norm", c)
    for n in ("query", "key", "value", "proj_attn"):
        _lin(spec, f"{a}.{n}", c, c)
    _resnet2d(spec, p + ".resnets.1", c, c)


def vae_param_spec(cfg: VAEConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """name -> shape of the diffusers-0.11.1 ``AutoencoderKL`` state dict (App. C.5)."""
    spec: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    boc = cfg.block_out_channels
    # encoder
    _conv(spec, "encoder.conv_in", boc[0], cfg.in_channels, 3)
    out_c = boc[0]
    for i in range(len(boc)):
        in_c, out_c = out_c, boc[i]
        for j in range(cfg.layers_per_block):
            _resnet2d(spec, f"encoder.down_blocks.{i}.resnets.{j}", in_c if j == 0 else out_c, out_c)
        if i != len(boc) - 1:
            _conv(spec, f"encoder.down_blocks.{i}.downsamplers.0.conv", out_c, out_c, 3)
    _vae_mid(spec, "encoder.mid_block", boc[-1])
    _norm(spec, "encoder.conv_norm_out", boc[-1])
    _conv(spec, "encoder.conv_out", 2 * cfg.latent_channels, boc[-1], 3)
    # decoder
    rev = list(reversed(boc))
    _conv(spec, "decoder.conv_in", rev[0], cfg.latent_channels, 3)
    _vae_mid(spec, "decoder.mid_block", rev[0])
    out_c = rev[0]
    for i in range(len(boc)):
        in_c, out_c = out_c, rev[i]
        for j in range(cfg.layers_per_block + 1):
            _resnet2d(spec, f"decoder.up_blocks.{i}.resnets.{j}", in_c if j == 0 else out_c, out_c)
        if i != len(boc) - 1:
            _conv(spec, f"decoder.up_blocks.{i}.upsamplers.0.conv", out_c, out_c, 3)
    _norm(spec, "decoder.conv_norm_out", boc[0])
    _conv(spec, "decoder.conv_out", cfg.out_channels, boc[0], 3)
    _conv(spec, "quant_conv", 2 * cfg.latent_channels, 2 * cfg.latent_channels, 1)
    _conv(spec, "post_quant_conv", cfg.latent_channels, cfg.latent_channels, 1)
    return spec


# --------------------------------------------------------------------------------------
# synthetic tensors
# --------------------------------------------------------------------------------------
def _is_norm(name: str) -> bool:
    leaf = name.rsplit(".", 2)[-2]
    return leaf.startswith("norm") or leaf.startswith("layer_norm") or leaf in ("group_norm", "conv_norm_out", "final_layer_norm")


def synth_tensor(name: str, shape: Tuple[int, ...], seed: int = 42, mode: str = "perturbed",
                 fan_in: int = 0) -> np.ndarray:
    """One synthetic parameter.

    ``mode="reference_init"``: torch-default-style init (``U(+-1/sqrt(fan_in))`` for conv and
    linear weight and bias; norm gamma=1, beta=0; ``attn_temp.to_out.0.weight`` = 0 as
    ``attention.py:201`` does) -- BASELINE config 1.
    ``mode="perturbed"``: same, but norm affine parameters are ``1 + 0.2u`` / ``0.2u`` and the
    temporal ``to_out`` weight is non-zero, so that no term of the path is hidden by a
    neutral parameter in a parity test.
    """
    n = int(np.prod(shape))
    if name.endswith("running_var"):       # a variance: positive, 0.5 .. 1.5
        return (0.5 + counter_uniform(seed, name, n)).astype(np.float32).reshape(shape)
    if _is_norm(name):
        if mode == "reference_init":
            v = np.ones(n, np.float32) if name.endswith(".weight") else np.zeros(n, np.float32)
        else:
            u = counter_uniform(seed, name, n) * 2.0 - 1.0
            v = (1.0 + 0.2 * u if name.endswith(".weight") else 0.2 * u).astype(np.float32)
        return v.reshape(shape)
    if mode == "reference_init" and name.endswith("attn_temp.to_out.0.weight"):
        return np.zeros(shape, np.float32)
    if name.endswith(".weight"):
        fan_in = int(np.prod(shape[1:]))
    elif fan_in <= 0:                      # bias without a known sibling weight
        fan_in = shape[0] if shape else 1
    bound = 1.0 / math.sqrt(max(fan_in, 1))
    u = counter_uniform(seed, name, n) * 2.0 - 1.0
    return (u * bound).astype(np.float32).reshape(shape)


def synth_state_dict(spec: "OrderedDict[str, Tuple[int, ...]]", seed: int = 42,
                     mode: str = "perturbed") -> "OrderedDict[str, np.ndarray]":
    """All tensors of ``spec`` (numpy float32), bias bounds taken from the sibling weight."""
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for name, shape in spec.items():
        fan_in = 0
        if name.endswith(".bias"):
            w = spec.get(name[:-5] + ".weight")
            if w is not None and len(w) > 1:
                fan_in = int(np.prod(w[1:]))
        out[name] = synth_tensor(name, shape, seed, mode, fan_in)
    return out


def synth_inputs(batch: int, cfg: UNetConfig, frames: int, h: int, w: int, n_tokens: int = 77,
                 seed: int = 1234):
    """BASELINE config-1 style inputs: latents ``[B,4,F,h,w]`` (seed+k per clip), cond and
    uncond ``[B,77,cross]`` / ``[1,77,cross]`` from their own seeds."""
    lat = np.stack([counter_normal(seed + k, "latent", (cfg.in_channels, frames, h, w)) for k in range(batch)])
    cond = np.stack([counter_normal(seed + 1 + 7919 * k, "cond", (n_tokens, cfg.cross_attention_dim))
                     for k in range(batch)])
    uncond = counter_normal(seed + 2, "uncond", (1, n_tokens, cfg.cross_attention_dim))
    return lat, cond, uncond
