"""Command-line flags of the training / inference entry points — the reference's config.py:3-45
(every one of its 31 flags, same names, types and defaults) plus the MI355X build's own:

  --config {c1,c2,c4,c5}   model/clip shapes of BASELINE.json's configurations (deepfake_amd.models.fused)
  --dtype {bf16,fp32}      compute precision (fp32 = the parity mode of the 1e-3 logits gate)
  --graph / --no-graph     replay the whole training step as one HIP graph (default on)
  --train_clips / --val_clips / --test_clips   size of the synthetic split (no media ships with the repo)
  --frames {normalized,uint8}   synthetic frames as the reference's transform output (fp32, ImageNet
                           normalised) or as decoded uint8 RGB frames normalised on the GPU
  --mel_source {image,uint8,wave,wave16k}   mel slot input: the reference's cached image (fp32 normalised, or
                           the uint8 grey image), a 22.05 kHz waveform, or the clip's own 16 kHz waveform (the same
                           samples wav2vec2 gets), resampled and turned into the mel image on the GPU
  --audio_seconds FLOAT    clip length of the waveform and mel slots in seconds, in place of the configuration's own
                           (wav2vec2 attention streams K / V through LDS past 640 frames, so 15 s or 30 s clips run)
  --audio_seconds_min      shortest synthetic clip (seconds): clips of unequal length, each mel image built from its
                           clip's own length on the GPU (default: one fixed length)
  --paudio_lengths         waveform slot with per-clip lengths (a layer-norm --w2v_config, or the wav2vec2-base one with
                           masked_group_norm, deepfake_amd/models/w2v_base_masked_config.json): each clip normalised
                           over its own samples, its padding masked in every wav2vec2 attention layer and left out of
                           the pooled feature; the padded waveform keeps the configuration's fixed length
  --bucket_mb              gradient all-reduce bucket size
  --deterministic          dropout / DropPath / SpecAugment / LayerDrop off (the parity setting, Q12)
  --optimizer {sgd,adamw}  the reference's SGD(momentum 0.9) (default) or the AdamW it keeps beside it
                           (src/trainer.py:78: betas (0.9, 0.999), weight decay --l2_decacy), fused on the device;
                           --adam_beta1, --adam_beta2, --adam_eps set its other hyper-parameters
  --clip_grad_norm FLOAT   global gradient-norm clipping (torch.nn.utils.clip_grad_norm_ on the mean gradient right
                           before the step) fused into either optimizer on the device; 0 (default): off
  --no_decay {none,norm_bias}   parameter groups of either optimizer: norm_bias takes 1-D parameters (norm gains,
                           biases) and the Swin position parameters (relative_position_bias_table, absolute_pos_embed,
                           cpb_mlp, logit_scale) out of --l2_decacy; none (default): the reference's single group
  --lr_scale PREFIX=MULT   learning-rate multiplier for the parameters whose name starts with PREFIX (the longest
                           matching prefix wins), repeatable: --lr_scale vExtract=0.1 --lr_scale aExtract=0.1
  --ema_decay FLOAT        exponential moving average of the weights, updated on the device right after every
                           optimizer step (inside the captured step); validation, submission and the checkpoint's
                           "checkpoint_ema" use the averaged weights; 0 (default): off.  --ema_warmup ramps the decay
                           as min(decay, (1 + n) / (10 + n)) over the first updates
  --video_encoder {swin,inception}   video slot: the north-star Video Swin 3D (default) or the reference's
                           current InceptionVideoClassifier (Inception-ResNet-v2 + NeXtVLAD, train.py:32,44)

Launch one process per GPU: python -m torch.distributed.run --nproc-per-node N train.py ...
"""
import argparse


def build_parser():
    parser = argparse.ArgumentParser(description="Deepfake")
    # DATA (config.py:6-11)
    parser.add_argument('--data_root', type=str, default=r'/data/lingfeng/full_data/phase1')
    parser.add_argument('--modality', type=str, default='audio')
    parser.add_argument('--num_frames', type=int, default=32, help='extract fixed number of frames')
    parser.add_argument('--force_generate', action='store_true', help='force process audio file')
    parser.add_argument('-nu', '--num_workers', type=int, default=1, help='thread number')
    # Model (config.py:13-28)
    parser.add_argument('--video_pretrained_dir', type=str,
                        default='checkpoints/swin_small_patch244_window877_kinetics400_1k.pth')
    parser.add_argument('--audio_pretrained_dir', type=str, default='checkpoints/swinv2_tiny_patch4_window16_256.pth')
    parser.add_argument('--classify_drop', type=float, default=0.1, help='MLP_dropout_rate')
    parser.add_argument('--swin_drop', type=float, default=0.1, help='VST_dropout_rate')
    parser.add_argument('--soft', type=float, default=0.01, help='NCE-SoftParam')
    parser.add_argument('--num_hiddens', type=int, default=128, help='Hidden Num of Classifier')
    parser.add_argument('--video_pool', type=str, help='VST Pool Method')
    parser.add_argument('--audio_ckpt_path', type=str, default=None)
    parser.add_argument('--video_ckpt_path', type=str, default=None)
    parser.add_argument('--paudio_ckpt_path', type=str, default=None)
    parser.add_argument('--fused_ckpt_path', type=str, default=None)
    parser.add_argument('--bn_momentum', type=float, default=0.1, help='BatchNorm Momentum')
    parser.add_argument('--Resume', action='store_true', help='resume model from ckpt')
    # Learning (config.py:30-41)
    parser.add_argument('--random_seed', type=int, default=42, help='torch random seed')
    parser.add_argument('-b', '--batch_size', type=int, default=8, help='input batch size for training (default: 32)')
    parser.add_argument('--accum_step', type=int, default=4, help='Gradient Accumulation Steps')
    parser.add_argument('-cuda', '--use_cuda', type=bool, default=True, help='Use cuda or not')
    parser.add_argument('--align_loss_rate', type=float, default=0.4, help='Ratio of Loss_align')
    parser.add_argument('--l2_decacy', type=float, default=0.05)
    parser.add_argument('-e', '--epochs', type=int, default=50, help='input training epoch for training (default: 50)')
    parser.add_argument('-lr', '--learning_rate', type=float, default=1e-4,
                        help='input learning rate for training (default: 1e-4)')
    parser.add_argument('--model_save', type=int, default=5, help='save model per %%d round')
    parser.add_argument('--skip_learning', action='store_true', help='skip train stage and get submission')
    parser.add_argument('--val_model', action='store_true', help='Eval Model Performence on Eval Set')
    # Log (config.py:43-44)
    parser.add_argument('--log_step', type=int, default=10)
    parser.add_argument('--log_dir', type=str, default=None)
    # MI355X build
    parser.add_argument('--config', type=str, default='c2', choices=['c1', 'c2', 'c4', 'c5'])
    parser.add_argument('--w2v_config', type=str, default=None, metavar='PATH',
                        help='wav2vec2 config JSON of the waveform slot (default: the wav2vec2-base one in '
                             'deepfake_amd/models/; deepfake_amd/models/w2v_large_config.json is the layer-norm / '
                             'pre-norm wav2vec2-large-lv60 layout); w2v_layers of --config still sets the layer count')
    parser.add_argument('--dtype', type=str, default='bf16', choices=['bf16', 'fp32'])
    parser.add_argument('--graph', dest='graph', action='store_true', default=True)
    parser.add_argument('--no-graph', dest='graph', action='store_false')
    parser.add_argument('--train_clips', type=int, default=64)
    parser.add_argument('--val_clips', type=int, default=16)
    parser.add_argument('--test_clips', type=int, default=16)
    parser.add_argument('--frames', type=str, default='normalized', choices=['normalized', 'uint8'])
    # f2 media front end on the device: mel slot input as the reference's cached image (fp32 normalised or the
    # uint8 grey image), as the raw 22.05 kHz waveform (device mel-spectrogram image) or as the clip's own 16 kHz
    # waveform (wave16k: resampled to 22.05 kHz on the device first); train-time frame augmentation (flips,
    # rotation) of uint8 frames on the device
    parser.add_argument('--mel_source', type=str, default='image', choices=['image', 'uint8', 'wave', 'wave16k'])
    parser.add_argument('--audio_seconds_min', type=float, default=None,
                        help='shortest clip in seconds: every clip draws its own audio length between this and the '
                             "configuration's (unequal clips per batch; the waveform mel sources then build each "
                             "image from its clip's own length).  Default: every clip has the configuration's length")
    parser.add_argument('--audio_seconds', type=float, default=None,
                        help="clip length in seconds of the waveform and mel slots (e.g. 30); default: the "
                             "configuration's own.  --audio_seconds_min and the padded width of --paudio_lengths follow")
    parser.add_argument('--paudio_lengths', action='store_true',
                        help="waveform slot: pass every clip's own length to wav2vec2 (per-clip normalisation, key "
                             'padding mask, pooling over the clip\'s frames); needs a layer-norm --w2v_config, or the '
                             'wav2vec2-base one with per-clip GroupNorm statistics, '
                             'deepfake_amd/models/w2v_base_masked_config.json')
    parser.add_argument('--augment', action='store_true')
    parser.add_argument('--bucket_dtype', type=str, default='fp32', choices=['fp32', 'bf16'])
    parser.add_argument('--bucket_mb', type=float, default=64.0)
    parser.add_argument('--deterministic', action='store_true')
    parser.add_argument('--video_encoder', type=str, default='swin', choices=['swin', 'inception'])
    parser.add_argument('--optimizer', type=str, default='sgd', choices=['sgd', 'adamw'],
                        help='fused device optimizer: SGD(momentum 0.9) or AdamW, both with --l2_decacy')
    parser.add_argument('--adam_beta1', type=float, default=0.9)
    parser.add_argument('--adam_beta2', type=float, default=0.999)
    parser.add_argument('--adam_eps', type=float, default=1e-8)
    parser.add_argument('--clip_grad_norm', type=float, default=0.0,
                        help='max global gradient norm (clip_grad_norm_ semantics, on the device); 0: no clipping')
    parser.add_argument('--no_decay', type=str, default='none', choices=['none', 'norm_bias'],
                        help='norm_bias: no weight decay on 1-D parameters and the Swin position parameters '
                             '(per-group weight decay in the fused optimizer); none: one group')
    parser.add_argument('--lr_scale', action='append', default=[], metavar='PREFIX=MULT',
                        help='learning-rate multiplier for the parameters whose name starts with PREFIX; repeatable, '
                             'the longest matching prefix wins')
    parser.add_argument('--ema_decay', type=float, default=0.0,
                        help='decay of the weight EMA kept on the device, in [0, 1) (e.g. 0.9999); validation, '
                             'submission and the checkpoint use the averaged weights; 0: no EMA')
    parser.add_argument('--ema_warmup', action='store_true',
                        help='ramp the EMA decay as min(ema_decay, (1 + n) / (10 + n)) after n updates')
    return parser


def get_opt(argv=None):
    return build_parser().parse_args(argv)


def audio_seconds(args, cfg):
    """The clip length in seconds: --audio_seconds, or the configuration's own."""
    sec = getattr(args, "audio_seconds", None)
    if sec is None:
        return cfg["seconds"]
    if not sec > 0:
        raise ValueError(f"--audio_seconds must be positive, got {sec}")
    return int(sec) if float(sec).is_integer() else float(sec)


def clip_seconds(args, cfg):
    """The synthetic clips' audio length for deepfake_amd.data.DeepFake: the fixed length (--audio_seconds, or the
    configuration's), or with --audio_seconds_min the pair (lo, hi) from which every clip draws its own."""
    hi = audio_seconds(args, cfg)
    lo = getattr(args, "audio_seconds_min", None)
    if lo is None:
        return hi
    if not 0 < lo <= hi:
        raise ValueError(f"--audio_seconds_min must lie in (0, {hi}], got {lo}")
    return (lo, hi)
