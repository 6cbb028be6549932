"""wav2vec2 (base, and the layer-norm / pre-norm large family) on MI355X with
HF-compatible state_dict keys (drop-in for the ``transformers.Wav2Vec2Model``
the reference builds at train.py:46 and wraps in Audio2D, audioTransformer.py:5-30).  Restates transformers 5.15.0
models/wav2vec2/modeling_wav2vec2.py (HF/ below) on HIP kernels:

  conv0 + GroupNorm + GELU        dfk_w2v_conv0_*   (HF/:302-323)
  conv1..6 + GELU                 implicit-GEMM conv (HF/:253-272), channels-last
  feature projection LN + Linear  (HF/:422-435)
  weight-normed grouped pos-conv  implicit GEMM per (clip, group), + residual (HF/:326-380,689)
  12 post-LN encoder layers       fused qkv GEMM, whole-sequence attention kernel,
                                  out_proj+residual, LN, FFN(+residual), LN (HF/:575-608)

With feat_extract_norm == "layer" and do_stable_layer_norm (wav2vec2-large-lv60, XLS-R, HuBERT-large configs):

  conv0 (+bias) + LayerNorm + GELU    dfk_w2v_conv0_ln_*  (HF/:275-299), one launch each way
  conv1..6 (+bias) + LayerNorm + GELU implicit-GEMM conv with a bias epilogue, then dfk_w2v_ln_gelu_*
  pre-LN encoder layers + final LN    the same ops in the other order (HF/:611-654, :729-802)

Training-mode regularisers of the checkpoint config (HF/ sites, all drawn on the
device, deepfake_amd.rng): feat_proj_dropout after the projection GEMM (:433),
SpecAugment time masking with masked_spec_embed (:1272-1317), hidden dropout
after the encoder-input LN (:692), attention-probability dropout inside the
attention kernel (:458), hidden dropout after out_proj and after the FFN output
GEMM (:596,:571), activation dropout after the FFN GELU (:568), all fused into
the producing kernel's epilogue; LayerDrop (:700-706) as per-layer device coins:
a dropped layer still runs (a captured graph cannot branch) but its output is
discarded (torch.where), its gradients are zero and the fused SGD skips its
parameters (as torch's SGD skips grad=None).  config.deterministic() turns all
of them off (the parity setting, Q12).

Padded batches: Wav2Vec2Model.forward(wave, lengths=n) gives every clip the result it would get alone —
frame_lengths() turns the sample counts into frame counts on the device, the hidden states past a clip's frames are
zeroed before the positional conv and after the encoder (Fn.RowMaskFn), every layer's attention masks the keys past
them (klen), and SpecAugment draws its spans inside them.  The lengths are never read on the host, so the step stays
capturable.  The layer-norm family takes lengths= as it is.  The group-norm family needs config.masked_group_norm
(w2v_base_masked_config.json; not an HF field): conv0's GroupNorm then takes each channel's mean and variance over
the clip's own frames (dfk_w2v_conv0_ragged_*), which is HF's arithmetic on the clip alone and not HF's on the padded
batch, where the padding enters every frame's statistics and no attention mask undoes it.  Without the field
lengths= raises on that family.
"""
import json

import torch
import torch.nn as nn
from torch.nn.utils import parametrizations

from .. import functional as Fn
from .. import kernels as K
from .. import rng


class Wav2Vec2Config:
    """The fields of HF Wav2Vec2Config this path reads (config.json of the
    reference checkpoint: checkpoints/wav2vec2-base-960h/config.json)."""

    def __init__(self, **kw):
        self.conv_dim = kw.get("conv_dim", [512] * 7)
        self.conv_kernel = kw.get("conv_kernel", [10, 3, 3, 3, 3, 2, 2])
        self.conv_stride = kw.get("conv_stride", [5, 2, 2, 2, 2, 2, 2])
        self.conv_bias = kw.get("conv_bias", False)
        self.feat_extract_norm = kw.get("feat_extract_norm", "group")
        self.hidden_size = kw.get("hidden_size", 768)
        self.num_attention_heads = kw.get("num_attention_heads", 12)
        self.intermediate_size = kw.get("intermediate_size", 3072)
        self.num_hidden_layers = kw.get("num_hidden_layers", 12)
        self.num_conv_pos_embeddings = kw.get("num_conv_pos_embeddings", 128)
        self.num_conv_pos_embedding_groups = kw.get("num_conv_pos_embedding_groups", 16)
        self.layer_norm_eps = kw.get("layer_norm_eps", 1e-5)
        self.do_stable_layer_norm = kw.get("do_stable_layer_norm", False)
        self.mask_time_prob = kw.get("mask_time_prob", 0.05)
        self.mask_time_length = kw.get("mask_time_length", 10)
        self.mask_time_min_masks = kw.get("mask_time_min_masks", 2)
        self.mask_feature_prob = kw.get("mask_feature_prob", 0.0)
        self.apply_spec_augment = kw.get("apply_spec_augment", True)
        self.layerdrop = kw.get("layerdrop", 0.1)
        # not an HF field: lengths= on the group-norm family, conv0's GroupNorm over each clip's own frames
        self.masked_group_norm = bool(kw.get("masked_group_norm", False))
        if self.masked_group_norm and self.feat_extract_norm != "group":
            raise ValueError(f"masked_group_norm with feat_extract_norm={self.feat_extract_norm!r}: the field selects "
                             'the padded-batch GroupNorm of feat_extract_norm="group" (the layer-norm family takes '
                             "lengths= without it)")
        for k in ("hidden_dropout", "attention_dropout", "activation_dropout", "feat_proj_dropout"):
            setattr(self, k, kw.get(k, 0.1))

    @classmethod
    def from_json_file(cls, path, **overrides):
        with open(path) as f:
            d = json.load(f)
        d.update(overrides)
        return cls(**d)

    def deterministic(self):
        """Parity / benchmark setting (Q12): dropouts, LayerDrop and SpecAugment off."""
        for k in ("hidden_dropout", "attention_dropout", "activation_dropout", "feat_proj_dropout", "layerdrop",
                  "mask_time_prob", "mask_feature_prob"):
            setattr(self, k, 0.0)
        return self


def frame_lengths(n, config):
    """Frames the conv stack gives for n samples (HF _get_feat_extract_output_lengths, :1059-1077):
    n <- (n - k_i) // s_i + 1 over the layers.  n: an integer tensor (integer torch ops on its device, no host
    read), a python integer, or a sequence of them (a list comes back)."""
    if not torch.is_tensor(n) and not isinstance(n, int):
        return [frame_lengths(int(v), config) for v in n]
    for k, s in zip(config.conv_kernel, config.conv_stride):
        n = torch.div(n - k, s, rounding_mode="floor") + 1 if torch.is_tensor(n) else (n - k) // s + 1
    return n


def padded_batches(config):
    """Whether the config has a padded-batch path (lengths=): the layer-norm / pre-norm family, or the group-norm
    family with masked_group_norm."""
    if config.feat_extract_norm == "layer":
        return bool(config.do_stable_layer_norm)
    return config.feat_extract_norm == "group" and bool(getattr(config, "masked_group_norm", False))


def receptive_field(config):
    """Samples behind one output frame of the conv stack (400 for the supported kernels and strides)."""
    r = 1
    for k, s in zip(reversed(config.conv_kernel), reversed(config.conv_stride)):
        r = (r - 1) * s + k
    return r


class _ConvLayer(nn.Module):
    """One feature-encoder layer's parameters under HF's names: ``norm`` is None (HF/:253-272), "group"
    (GroupNorm, HF/:302-323) or "layer" (LayerNorm over the channels of each frame, HF/:275-299; built without
    an eps argument there, so nn.LayerNorm's default 1e-5 and not config.layer_norm_eps)."""

    def __init__(self, cin, cout, k, s, norm, bias=False):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, kernel_size=k, stride=s, bias=bias)
        if norm == "group":
            self.layer_norm = nn.GroupNorm(num_groups=cout, num_channels=cout, affine=True)
        elif norm == "layer":
            self.layer_norm = nn.LayerNorm(cout, elementwise_affine=True)
        self.stride = s


class Wav2Vec2FeatureEncoder(nn.Module):
    """HF/:382-419: feat_extract_norm == "group" (wav2vec2-base: GroupNorm on layer 0 only, no conv bias) or
    "layer" (wav2vec2-large-lv60 / XLS-R / HuBERT-large: LayerNorm on all seven layers, conv_bias either way)."""

    def __init__(self, config):
        super().__init__()
        if config.feat_extract_norm not in ("group", "layer"):
            raise NotImplementedError(f"feat_extract_norm {config.feat_extract_norm!r}")
        if config.feat_extract_norm == "group" and config.conv_bias:
            raise NotImplementedError("group-norm feature encoder with conv_bias")
        if config.conv_dim[0] != 512 or config.conv_kernel[0] != 10 or config.conv_stride[0] != 5:
            raise NotImplementedError("only a 512x10/5 conv0")
        self.layer_norm_path = config.feat_extract_norm == "layer"
        if self.layer_norm_path and any(d != 512 for d in config.conv_dim):
            raise NotImplementedError("layer-norm feature encoder with a conv_dim other than 512")
        dims = [1] + list(config.conv_dim)
        if self.layer_norm_path:
            self.conv_layers = nn.ModuleList([
                _ConvLayer(dims[i], dims[i + 1], config.conv_kernel[i], config.conv_stride[i], "layer",
                           bool(config.conv_bias))
                for i in range(len(config.conv_dim))])
        else:
            self.conv_layers = nn.ModuleList([
                _ConvLayer(dims[i], dims[i + 1], config.conv_kernel[i], config.conv_stride[i],
                           "group" if i == 0 else None)
                for i in range(len(config.conv_dim))])
        self.compute_dtype = torch.float32

    def forward(self, input_values, lengths=None):
        """[B, S] fp32 -> channels-last [B, T, 512] (compute dtype).  lengths (device int64 [B], group path): conv0
        over each clip's own samples and frames, zero rows behind them; conv1..6 carry no bias and gelu(0) = 0, so
        the frames that see padding only stay zero, and those that straddle a clip's end lie at or past its frame
        count, where the encoder's row mask removes them."""
        l0 = self.conv_layers[0]
        if self.layer_norm_path:
            x = Fn.W2VConv0LNFn.apply(input_values, l0.conv.weight, l0.conv.bias, l0.layer_norm.weight,
                                      l0.layer_norm.bias, l0.layer_norm.eps, self.compute_dtype)
            for layer in self.conv_layers[1:]:
                x = Fn.ConvLNGeluFn.apply(x, layer.conv.weight, layer.conv.bias, layer.layer_norm.weight,
                                          layer.layer_norm.bias, layer.stride, layer.layer_norm.eps)
            return x
        if lengths is None:
            x = Fn.W2VConv0Fn.apply(input_values, l0.conv.weight, l0.layer_norm.weight, l0.layer_norm.bias,
                                    l0.layer_norm.eps, self.compute_dtype)
        else:
            x = Fn.W2VConv0Fn.apply(input_values, l0.conv.weight, l0.layer_norm.weight, l0.layer_norm.bias,
                                    l0.layer_norm.eps, self.compute_dtype, lengths)
        for layer in self.conv_layers[1:]:
            x = Fn.ConvGeluFn.apply(x, layer.conv.weight, layer.stride)
        return x


class Wav2Vec2FeatureProjection(nn.Module):
    """HF/:422-435."""

    def __init__(self, config):
        super().__init__()
        self.layer_norm = nn.LayerNorm(config.conv_dim[-1], eps=config.layer_norm_eps)
        self.projection = nn.Linear(config.conv_dim[-1], config.hidden_size)
        self.dropout = rng.Drop(config.feat_proj_dropout)

    def forward(self, x):
        n = Fn.layer_norm(x, self.layer_norm)
        d = self.dropout.spec() if self.dropout.active(self.training) else None
        return Fn.linear(n, self.projection.weight, self.projection.bias, drop=d), n


class Wav2Vec2PositionalConvEmbedding(nn.Module):
    """HF/:326-368 (weight-norm dim=2; SamePad drops the last frame)."""

    def __init__(self, config):
        super().__init__()
        conv = nn.Conv1d(config.hidden_size, config.hidden_size, kernel_size=config.num_conv_pos_embeddings,
                         padding=config.num_conv_pos_embeddings // 2, groups=config.num_conv_pos_embedding_groups)
        self.conv = parametrizations.weight_norm(conv, name="weight", dim=2)
        self.groups = config.num_conv_pos_embedding_groups
        if config.num_conv_pos_embeddings % 2:
            raise NotImplementedError("odd num_conv_pos_embeddings")

    def weight(self):
        """weight_norm(dim=2): g * v / ||v|| with the norm over dims (0, 1) — same parameters and state_dict
        keys as the parametrization, composed from plain reductions.  The tests' reference of the positional
        conv reads it; the model's path is add_to() (the torch route through this and Fn.PosConvFn lost the step
        A/B, profiles/step/r6x_posconv_weightnorm.txt)."""
        p = self.conv.parametrizations.weight
        g, v = p.original0, p.original1
        return v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())

    def add_to(self, x):
        """x + pos_conv(x) fused (HF/:689-690), the weight norm inside the op (Fn.PosConvWNFn)."""
        p = self.conv.parametrizations.weight
        return Fn.PosConvWNFn.apply(x, p.original0, p.original1, self.conv.bias, self.groups)


class Wav2Vec2Attention(nn.Module):
    """HF/:466-548: q/k/v/out projections; softmax(q k^T * hd^-0.5) v."""

    def __init__(self, embed_dim, num_heads, dropout=0.0):
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.dropout = rng.Drop(dropout)
        self.head_dim = embed_dim // num_heads
        self.scaling = self.head_dim ** -0.5
        self.k_proj = nn.Linear(embed_dim, embed_dim)
        self.v_proj = nn.Linear(embed_dim, embed_dim)
        self.q_proj = nn.Linear(embed_dim, embed_dim)
        self.out_proj = nn.Linear(embed_dim, embed_dim)

    def flat_groups(self):
        """ParamStore adjacency: q/k/v weights and biases back to back -> one fused qkv GEMM operand."""
        q, k, v = self.q_proj, self.k_proj, self.v_proj
        return [[q.weight, k.weight, v.weight], [q.bias, k.bias, v.bias]]

    def core(self, x, B, T, skip=False, klen=None):
        """x [B*T, C] -> attention output [B*T, C] before out_proj (skip=True: and an alias of x for the
        layer's residual, whose gradient joins the q/k/v dX GEMM).  klen: int32 [B] device tensor of each clip's
        frames (padded batches): keys past them are masked, rows past them come out as zero."""
        q, k, v = self.q_proj, self.k_proj, self.v_proj
        qkv = Fn.linear_group(x, (q.weight, k.weight, v.weight), (q.bias, k.bias, v.bias), skip=skip)
        if skip:
            qkv, xs = qkv
        geo = ((B, 1, 1, T), (1, 1, T), (1, 1, T), (0, 0, 0), self.num_heads, self.head_dim, self.scaling)
        d = self.dropout.spec() if self.dropout.active(self.training) else None
        out = Fn.window_attention(qkv, None, None, geo, drop=d, klen=klen)
        return (out, xs) if skip else out


class Wav2Vec2FeedForward(nn.Module):
    """HF/:551-573."""

    def __init__(self, config):
        super().__init__()
        self.intermediate_dense = nn.Linear(config.hidden_size, config.intermediate_size)
        self.output_dense = nn.Linear(config.intermediate_size, config.hidden_size)
        self.intermediate_dropout = rng.Drop(config.activation_dropout)
        self.output_dropout = rng.Drop(config.hidden_dropout)


class Wav2Vec2EncoderLayer(nn.Module):
    """HF/:575-608 (post-LN)."""

    def __init__(self, config):
        super().__init__()
        self.attention = Wav2Vec2Attention(config.hidden_size, config.num_attention_heads, config.attention_dropout)
        self.dropout = rng.Drop(config.hidden_dropout)
        self.layer_norm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.feed_forward = Wav2Vec2FeedForward(config)
        self.final_layer_norm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)

    def forward(self, x, B, T, klen=None):
        tr = self.training
        ff = self.feed_forward
        spec = lambda d: d.spec() if d.active(tr) else None   # noqa: E731
        a, xs = self.attention.core(x, B, T, skip=True, klen=klen)
        x = Fn.layer_norm(Fn.linear(a, self.attention.out_proj.weight, self.attention.out_proj.bias, residual=xs,
                                    drop=spec(self.dropout)), self.layer_norm)
        x = Fn.mlp(x, ff.intermediate_dense, ff.output_dense, residual=x, drop_act=spec(ff.intermediate_dropout),
                   drop_out=spec(ff.output_dropout))
        return Fn.layer_norm(x, self.final_layer_norm)


class Wav2Vec2Encoder(nn.Module):
    """HF/:657-727.  flen (device int64 [B], padded batches): the frames past a clip's own are zeroed before the
    positional conv (HF/:678-681), every layer's attention masks them as keys, and the output's rows there are
    zeroed (HF leaves the last LayerNorm's output in them)."""

    layer_class = Wav2Vec2EncoderLayer

    stable_layer_norm = False   # the config's do_stable_layer_norm this class implements

    def __init__(self, config):
        super().__init__()
        if bool(config.do_stable_layer_norm) != self.stable_layer_norm:
            raise NotImplementedError(f"{type(self).__name__} with do_stable_layer_norm={config.do_stable_layer_norm}"
                                      " (Wav2Vec2Model picks the encoder class by it)")
        self.pos_conv_embed = Wav2Vec2PositionalConvEmbedding(config)
        self.layer_norm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.dropout = rng.Drop(config.hidden_dropout)
        self.layers = nn.ModuleList([self.layer_class(config) for _ in range(config.num_hidden_layers)])
        # LayerDrop coins: rank-independent draws (every replica drops the same layers, so the SGD skip of a
        # dropped layer's parameters stays identical across data-parallel ranks); 1 = run, 0 = skip
        self.layerdrop = rng.Drop(config.layerdrop, shared=True)
        self.register_buffer("layer_keep", torch.ones(config.num_hidden_layers), persistent=False)
        # OR of the coins since the last zero_grad (the SGD gate): with gradient accumulation a layer kept in
        # any micro-step of the window has a gradient in the reference (p.grad is not None) and is stepped
        self.register_buffer("layer_used", torch.zeros(config.num_hidden_layers), persistent=False)

    def param_gates(self):
        """(parameters, device flag) pairs for the fused SGD: a layer's parameters are stepped only when its
        LayerDrop coin kept it in some micro-step since the last zero_grad (training with layerdrop > 0)."""
        if self.layerdrop.p <= 0:
            return []
        return [(list(l.parameters()), self.layer_used[i:i + 1]) for i, l in enumerate(self.layers)]

    def reset_gates(self):
        """Called with zero_grad (ParamStore.zero_gates): a new accumulation window starts with no layer kept."""
        self.layer_used.zero_()

    def forward(self, h, flen=None):
        B, T, C = h.shape
        klen = None
        if flen is not None:
            h = Fn.RowMaskFn.apply(h, flen)
            klen = flen.clamp(1, T).to(torch.int32)
        d = self.dropout.spec() if self.dropout.active(self.training) else None
        x = Fn.layer_norm(self.pos_conv_embed.add_to(h.contiguous()), self.layer_norm, drop=d).reshape(B * T, C)
        y = self._run_layers(x, B, T, klen).view(B, T, C)
        return y if flen is None else Fn.RowMaskFn.apply(y, flen)

    def _run_layers(self, x, B, T, klen=None):
        """The layers on x [B*T, C] under LayerDrop (HF/:700-706); klen: the layers' key lengths."""
        lds = self.layerdrop.active(self.training)
        if lds:
            K.layerdrop_flags(self.layerdrop.spec(), self.layer_keep, self.layer_used)
        for i, layer in enumerate(self.layers):
            y = layer(x, B, T) if klen is None else layer(x, B, T, klen)
            if not lds:
                x = y
            elif x.is_cuda and y.dtype == x.dtype and (y.numel() * y.element_size()) % 16 == 0:
                x = Fn.LayerSelectFn.apply(y, x, self.layer_keep[i:i + 1])
            else:
                x = torch.where(self.layer_keep[i] > 0, y, x)
        return x


class Wav2Vec2EncoderLayerStableLayerNorm(Wav2Vec2EncoderLayer):
    """HF/:611-654 (pre-LN; do_stable_layer_norm): the modules and parameter names of the post-LN layer in another
    order, h = h + dropout(out_proj(attn(layer_norm(h)))); h = h + FF(final_layer_norm(h)).  Each residual reads
    its LayerNorm's skip alias, so h's two gradients meet inside the LN backward (as the Swin pre-norm blocks)."""

    def forward(self, x, B, T, klen=None):
        tr = self.training
        ff = self.feed_forward
        spec = lambda d: d.spec() if d.active(tr) else None   # noqa: E731
        xn, xs = Fn.layer_norm(x, self.layer_norm, skip=True)
        a = self.attention.core(xn, B, T, klen=klen)
        x = Fn.linear(a, self.attention.out_proj.weight, self.attention.out_proj.bias, residual=xs,
                      drop=spec(self.dropout))
        xn, xs = Fn.layer_norm(x, self.final_layer_norm, skip=True)
        return Fn.mlp(xn, ff.intermediate_dense, ff.output_dense, residual=xs, drop_act=spec(ff.intermediate_dropout),
                      drop_out=spec(ff.output_dropout))


class Wav2Vec2EncoderStableLayerNorm(Wav2Vec2Encoder):
    """HF/:729-802: h + pos_conv(h) -> dropout -> pre-LN layers under LayerDrop -> encoder.layer_norm.  Parameter
    names, LayerDrop coins and SGD gates as the post-LN encoder.  flen (device int64 [B], padded batches): the
    frames past a clip's own are zeroed before the positional conv (HF/:761-764) and after the final LayerNorm
    (HF leaves that LayerNorm's output there), and every layer's attention masks them as keys."""

    layer_class = Wav2Vec2EncoderLayerStableLayerNorm
    stable_layer_norm = True

    def forward(self, h, flen=None):
        B, T, C = h.shape
        klen = None
        if flen is not None:
            h = Fn.RowMaskFn.apply(h, flen)
            klen = flen.clamp(1, T).to(torch.int32)
        x = self.pos_conv_embed.add_to(h.contiguous()).reshape(B * T, C)
        if self.dropout.active(self.training):
            x = Fn.DropoutFn.apply(x, self.dropout.spec())
        y = Fn.layer_norm(self._run_layers(x, B, T, klen), self.layer_norm).view(B, T, C)
        return y if flen is None else Fn.RowMaskFn.apply(y, flen)


class Wav2Vec2Model(nn.Module):
    """HF/:1244-1380 forward.  config.do_stable_layer_norm picks the encoder (HF/:1255) and
    config.feat_extract_norm the feature encoder.  Padded batches come with lengths= (the samples of each clip, an
    int64 [B] device tensor that is never read on the host, or host integers, which are validated): the layer-norm
    family, and the group-norm family with config.masked_group_norm; HF's attention_mask argument raises."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.feature_extractor = Wav2Vec2FeatureEncoder(config)
        self.feature_projection = Wav2Vec2FeatureProjection(config)
        if config.mask_time_prob > 0.0 or config.mask_feature_prob > 0.0:
            self.masked_spec_embed = nn.Parameter(torch.empty(config.hidden_size).uniform_())
        self.encoder = (Wav2Vec2EncoderStableLayerNorm if config.do_stable_layer_norm else Wav2Vec2Encoder)(config)

        self.spec_site = rng.Drop(0.0)   # SpecAugment draws (site only)
        if config.mask_feature_prob > 0.0:
            raise NotImplementedError("SpecAugment feature masking (mask_feature_prob > 0)")

    def _mask_hidden_states(self, h, flen=None):
        """HF/:1272-1317 time masking (training, apply_spec_augment, mask_time_prob > 0); flen: the spans of each
        clip inside its own frames."""
        c = self.config
        if not (self.training and c.apply_spec_augment and c.mask_time_prob > 0):
            return h
        if flen is None:
            return Fn.SpecAugmentFn.apply(h, self.masked_spec_embed, c.mask_time_prob, c.mask_time_length,
                                          c.mask_time_min_masks, self.spec_site.spec())
        return Fn.SpecAugmentFn.apply(h, self.masked_spec_embed, c.mask_time_prob, c.mask_time_length,
                                      c.mask_time_min_masks, self.spec_site.spec(), flen)

    def sample_lengths(self, input_values, lengths):
        """lengths= of forward() as an int64 [B] tensor on the waveform's device.  A device tensor is checked for
        shape and dtype only (its values are clamped by the kernels that read them); host integers must lie in
        [receptive field, S]."""
        if not padded_batches(self.config):
            raise NotImplementedError("lengths= (padded batches) with the group-norm / post-LN family: its conv0 "
                                      "GroupNorm runs over the whole padded row (masked_group_norm in the config "
                                      "selects the per-clip statistics)")
        B, S = input_values.shape
        if torch.is_tensor(lengths) and lengths.is_cuda:
            if lengths.dtype != torch.int64 or lengths.shape != (B,):
                raise ValueError(f"lengths: int64 [{B}] expected, got {lengths.dtype} {tuple(lengths.shape)}")
            return lengths.contiguous()
        n = torch.as_tensor(lengths)
        if n.dtype not in (torch.int64, torch.int32, torch.int16, torch.uint8, torch.int8):
            raise ValueError(f"lengths: integers expected, got {n.dtype}")
        if n.shape != (B,):
            raise ValueError(f"lengths: [{B}] expected, got {tuple(n.shape)}")
        lo = receptive_field(self.config)
        if int(n.min()) < lo or int(n.max()) > S:
            raise ValueError(f"lengths: values in [{lo}, {S}] expected, got {n.tolist()}")
        return n.to(torch.int64).to(input_values.device)

    def forward(self, input_values, attention_mask=None, lengths=None, **_):
        if attention_mask is not None:
            raise NotImplementedError("attention_mask (padded batches): pass lengths=")
        flen = None
        if lengths is not None:
            lengths = self.sample_lengths(input_values, lengths)
            flen = frame_lengths(lengths, self.config)
        if lengths is not None and not self.feature_extractor.layer_norm_path:
            f = self.feature_extractor(input_values, lengths)
        else:   # the layer-norm conv stack is per frame: its padded frames are removed by the encoder's row mask
            f = self.feature_extractor(input_values)
        h, ext = self.feature_projection(f)
        h = self._mask_hidden_states(h, flen)
        h = self.encoder(h) if flen is None else self.encoder(h, flen)
        return {"last_hidden_state": h, "extract_features": ext}
