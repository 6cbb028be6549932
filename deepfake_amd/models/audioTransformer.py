"""Audio2D — drop-in for /root/reference/src/models/audioTransformer.py:5-30."""
import torch.nn as nn
import torch.nn.functional as F

from .. import functional as Fn
from ..utils import Mlp


class Audio2D(nn.Module):
    """wav_model(x).last_hidden_state -> mean over frames (AdaptiveAvgPool2d((1,in_feat)))
    -> F.dropout(p=args.swin_drop) — always on, as the reference (Q9) -> [B, in_feat]
    fp32 (use_feat=True); or the classifier branch (use_feat=False).  Padded batches: lengths= (or x as the pair
    (wave, lengths), the form a flat feature tuple carries) goes to the wav2vec2 model, and the mean runs over each
    clip's own frames."""

    def __init__(self, args, wav_model, in_feat=768, num_classes=2, use_feat=False):
        super().__init__()
        self.wav_model = wav_model
        self.use_feat = use_feat
        self.classifier = nn.Linear(512, num_classes)   # Q10: exists (unused) when use_feat=True
        self.model_drop = args.swin_drop
        if not use_feat:
            self.mlp = Mlp(in_feat, 512, 512)
            self.norm = nn.LayerNorm(512)
            self.act = nn.GELU()
            self.classify_drop = args.classify_drop

    def forward(self, x, mask=None, lengths=None):
        if isinstance(x, (tuple, list)):
            x, lengths = x
        if lengths is None:
            h = self.wav_model(x)["last_hidden_state"]
            B, T, C = h.shape
            feat = Fn.RowMeanFn.apply(h.reshape(B * T, C), B)
        else:
            from .wav2vec2 import frame_lengths
            n = self.wav_model.sample_lengths(x, lengths)
            h = self.wav_model(x, lengths=n)["last_hidden_state"]
            feat = Fn.RowMeanRaggedFn.apply(h, frame_lengths(n, self.wav_model.config))
        if self.model_drop > 0:
            feat = F.dropout(feat, self.model_drop)
        if not self.use_feat:
            c = self.act(self.norm(self.mlp(feat)))
            if self.classify_drop > 0:
                c = F.dropout(c, self.classify_drop)
            return self.classifier(c).squeeze().sigmoid()
        return feat
