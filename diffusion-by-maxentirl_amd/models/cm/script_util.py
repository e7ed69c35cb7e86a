"""`models.cm.script_util` — model/diffusion factory with the reference keyword surface
(reference: models/cm/script_util.py:10-219).  YAML `diffusion:` blocks written for the reference
instantiate unchanged: create_model_and_diffusion(**cfg.diffusion).  cm_train_defaults and create_ema_and_scales_fn are the
consistency-training side (models.cm.train_util.CMTrainLoop); `loss_norm` is set on the diffusion object by the caller.
"""
import argparse

import numpy as np

from .karras_diffusion import KarrasDenoiser
from .unet import UNetModel

NUM_CLASSES = 1000


def cm_train_defaults():
    """The reference's keys and values (:10-23), but loss_norm "l2": no LPIPS weights ship with this package, and the
    defaults must run without any.  "lpips" (the reference's default) is available once the caller supplies them (models.cm.lpips)."""
    return dict(teacher_model_path="", teacher_dropout=0.1, training_mode="consistency_distillation", target_ema_mode="fixed",
                scale_mode="fixed", total_training_steps=600000, start_ema=0.0, start_scales=40, end_scales=40,
                distill_steps_per_iter=50000, loss_norm="l2")


def model_and_diffusion_defaults():
    return dict(sigma_min=0.002, sigma_max=80.0, image_size=64, num_channels=128, num_res_blocks=2, num_heads=4,
                num_heads_upsample=-1, num_head_channels=-1, attention_resolutions="32,16,8", channel_mult="",
                dropout=0.0, class_cond=False, use_checkpoint=False, use_scale_shift_norm=True, resblock_updown=False,
                use_fp16=False, use_new_attention_order=False, learn_sigma=False, weight_schedule="karras")


def create_model_and_diffusion(image_size, class_cond, learn_sigma, num_channels, num_res_blocks, channel_mult, num_heads,
                               num_head_channels, num_heads_upsample, attention_resolutions, dropout, use_checkpoint,
                               use_scale_shift_norm, resblock_updown, use_fp16, use_new_attention_order, weight_schedule,
                               sigma_min=0.002, sigma_max=80.0, distillation=False):
    model = create_model(image_size, num_channels, num_res_blocks, channel_mult=channel_mult, learn_sigma=learn_sigma,
                         class_cond=class_cond, use_checkpoint=use_checkpoint, attention_resolutions=attention_resolutions,
                         num_heads=num_heads, num_head_channels=num_head_channels, num_heads_upsample=num_heads_upsample,
                         use_scale_shift_norm=use_scale_shift_norm, dropout=dropout, resblock_updown=resblock_updown,
                         use_fp16=use_fp16, use_new_attention_order=use_new_attention_order)
    diffusion = KarrasDenoiser(sigma_data=0.5, sigma_max=sigma_max, sigma_min=sigma_min, distillation=distillation,
                               weight_schedule=weight_schedule)
    return model, diffusion


def create_model(image_size, num_channels, num_res_blocks, channel_mult="", learn_sigma=False, class_cond=False,
                 use_checkpoint=False, attention_resolutions="16", num_heads=1, num_head_channels=-1, num_heads_upsample=-1,
                 use_scale_shift_norm=False, dropout=0, resblock_updown=False, use_fp16=False, use_new_attention_order=False):
    if channel_mult == "":
        table = {512: (0.5, 1, 1, 2, 2, 4, 4), 256: (1, 1, 2, 2, 4, 4), 128: (1, 1, 2, 3, 4), 64: (1, 2, 3, 4)}
        if image_size not in table:
            raise ValueError(f"unsupported image size: {image_size}")
        channel_mult = table[image_size]
    else:
        channel_mult = tuple(int(m) for m in str(channel_mult).split(","))
    attention_ds = tuple(image_size // int(res) for res in str(attention_resolutions).split(","))   # str(): a CLI override "16" arrives as int
    return UNetModel(image_size=image_size, in_channels=3, model_channels=num_channels,
                     out_channels=(3 if not learn_sigma else 6), num_res_blocks=num_res_blocks,
                     attention_resolutions=attention_ds, dropout=dropout, channel_mult=channel_mult,
                     num_classes=(NUM_CLASSES if class_cond else None), use_checkpoint=use_checkpoint, use_fp16=use_fp16,
                     num_heads=num_heads, num_head_channels=num_head_channels, num_heads_upsample=num_heads_upsample,
                     use_scale_shift_norm=use_scale_shift_norm, resblock_updown=resblock_updown,
                     use_new_attention_order=use_new_attention_order)


def create_ema_and_scales_fn(target_ema_mode, start_ema, scale_mode, start_scales, end_scales, total_steps, distill_steps_per_iter):
    """step -> (target EMA rate: float, num_scales: int) for the reference's four (target_ema_mode, scale_mode) pairs (:161-219),
    and ("fixed", "ict"): the doubling curriculum of improved consistency training (Song and Dhariwal 2023, section 3.4),
    N(k) = min(start_scales 2^(k // K'), end_scales) + 1 levels with K' = total_steps // (floor(log2(end_scales // start_scales)) + 1),
    at the fixed rate start_ema (0 there: the target is the stop-gradient student)."""
    pair = (target_ema_mode, scale_mode)
    if pair not in (("fixed", "fixed"), ("fixed", "progressive"), ("adaptive", "progressive"), ("fixed", "progdist"), ("fixed", "ict")):
        raise NotImplementedError(f"target_ema_mode={target_ema_mode!r} with scale_mode={scale_mode!r}")
    if pair == ("fixed", "ict"):
        if not (int(start_scales) >= 1 and int(end_scales) >= int(start_scales)):
            raise ValueError(f"scale_mode='ict': 1 <= start_scales <= end_scales is needed, got {start_scales}, {end_scales}")
        doublings = int(np.floor(np.log2(int(end_scales) // int(start_scales))))
        k_prime = max(1, int(total_steps) // (doublings + 1))

    def progressive_scales(step):
        scales = np.ceil(np.sqrt((step / total_steps) * ((end_scales + 1) ** 2 - start_scales ** 2) + start_scales ** 2) - 1).astype(np.int32)
        return np.maximum(scales, 1)

    def ema_and_scales_fn(step):
        if pair == ("fixed", "fixed"):
            target_ema, scales = start_ema, start_scales
        elif pair == ("fixed", "progressive"):
            target_ema, scales = start_ema, progressive_scales(step) + 1
        elif pair == ("fixed", "ict"):      # python ints: 2 ** (step // K') has no upper bound in a long run
            target_ema = start_ema
            scales = (int(end_scales) if int(step) // k_prime > doublings else min(int(start_scales) << (int(step) // k_prime), int(end_scales))) + 1
        elif pair == ("adaptive", "progressive"):
            scales = progressive_scales(step)
            c = -np.log(start_ema) * start_scales
            target_ema = np.exp(-c / scales)
            scales = scales + 1
        else:
            distill_stage = step // distill_steps_per_iter
            scales = np.maximum(start_scales // (2 ** distill_stage), 2)
            sub_stage = np.maximum(step - distill_steps_per_iter * (np.log2(start_scales) - 1), 0)
            sub_stage = sub_stage // (distill_steps_per_iter * 2)
            sub_scales = np.maximum(2 // (2 ** sub_stage), 1)
            scales = np.where(scales == 2, sub_scales, scales)
            target_ema = 1.0
        return float(target_ema), int(scales)

    return ema_and_scales_fn


def add_dict_to_argparser(parser, default_dict):
    for k, v in default_dict.items():
        v_type = str if v is None else (str2bool if isinstance(v, bool) else type(v))
        parser.add_argument(f"--{k}", default=v, type=v_type)


def args_to_dict(args, keys):
    return {k: getattr(args, k) for k in keys}


def str2bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("boolean value expected")
