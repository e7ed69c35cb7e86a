"""Every forward launch of the sampling and training programs against an fp64 reference, at the shapes the programs use.

CASES is the census of the forward launches (tests/forward_census.py) of the fourteen programs of forward_census.PROGRAMS:
CIFAR-10 generation at 256 / 32 (T=10) and 128 (T=4), CIFAR-10 training at 256 / 128 / 32 (throughput tuning), ImageNet-64
class-conditional generation at 100, ImageNet-64 training at 16 (throughput tuning), LSUN-256 generation at 16, and on the
full-size ImageNet-64 EDM net under the default knobs: DSM training (models/cm/train_util.TrainLoop) at 16 and 32 images,
the Karras Heun teacher sampler at 100, consistency multistep sampling (ts 0, 22, 39) at 100 and zero-shot inpainting at 14.
The two samplers at 100 add no network row to the table: they launch what imagenet64_sample_b100 launches, and
test_census_is_covered now guards that.  test_census_is_covered re-records each program and fails on any launch the table
lacks and on any `ops` function called outside a backward that is neither a launch op nor on the census's allow-lists.
test_every_row_kind_has_a_test keeps the row kinds of the table and the kinds the tests parametrise over equal.  Every row is then run on seeded
inputs and checked element by element (attention: also per 128-row block) against stock torch in float64 on the device, with the
bounds derived in tests/forward_bounds.py; conv rows run under the tuning the census recorded and must select the kernel the
census saw.  EXTRA rows reach the forward kernel instances no program launches, so that every conv kernel id
bench.kernel_name can name, both linear forms, every attention kernel and every GroupNorm path is launched here.

GroupNorm inputs carry one mean offset per group: the largest (image, group) |mean| / std of every image is COND_MULT times the
largest the census measured on the programs' own activations (random-init nets, not trained weights), at least MIN_COND.
"""
import json
import os
import zlib

import pytest
import torch

from backward_bounds import U16, U32, dropout_ref, groupnorm_bwd_ref, td_loss_ref
from forward_bounds import (MIN_COND, FwdChecker, attention_ref, attn_blocks, attn_elem_bound, block_stats_tensor, conv_call_ref, dsm_error_terms,
                            dsm_loss_fwd_bound, edm_step_ref, fold_passes, gn_bound, gn_fused_bound, gn_fwd_checked, gn_input, gn_ref,
                            linear_ref, log_sigma_t, lse_bound,
                            pool_act_ref, scaled_input_ref, stats_depth, stats_ref, store_bound, td_gather_cost_ref, var_step_ref)

DEV = "cuda:0"
CHECK = FwdChecker()
COND_MULT = 4.0

import forward_census  # noqa: E402
from forward_census import PROGRAMS  # noqa: E402
# The census (forward_census.record over every program), sorted and de-duplicated; COND: largest |mean| / std per GroupNorm row
CASES = [
    ('attention', 100, 1024, 384, 6, False, False, 'attention64'),
    ('attention', 100, 256, 576, 9, False, False, 'attention64'),
    ('attention', 100, 64, 768, 12, False, False, 'attention_kernel<64>'),
    ('attention', 128, 16, 256, 1, False, False, 'attention_kernel<256>'),
    ('attention', 128, 256, 256, 1, False, False, 'attention256<false>'),
    ('attention', 14, 1024, 384, 6, False, False, 'attention64'),
    ('attention', 14, 256, 576, 9, False, False, 'attention64'),
    ('attention', 14, 64, 768, 12, False, False, 'attention_kernel<64>'),
    ('attention', 16, 1024, 384, 6, False, False, 'attention64'),
    ('attention', 16, 1024, 384, 6, True, True, 'attention64'),
    ('attention', 16, 1024, 512, 8, False, False, 'attention64'),
    ('attention', 16, 256, 1024, 16, False, False, 'attention64'),
    ('attention', 16, 256, 576, 9, False, False, 'attention64'),
    ('attention', 16, 256, 576, 9, True, True, 'attention64'),
    ('attention', 16, 64, 1024, 16, False, False, 'attention_kernel<64>'),
    ('attention', 16, 64, 768, 12, False, False, 'attention_kernel<64>'),
    ('attention', 16, 64, 768, 12, True, True, 'attention_kernel<64>'),
    ('attention', 256, 16, 256, 1, False, False, 'attention_kernel<256>'),
    ('attention', 256, 256, 256, 1, False, False, 'attention256<false>'),
    ('attention', 32, 1024, 384, 6, True, True, 'attention64'),
    ('attention', 32, 16, 256, 1, False, False, 'attention_kernel<256>'),
    ('attention', 32, 256, 256, 1, False, False, 'attention256<false>'),
    ('attention', 32, 256, 576, 9, True, True, 'attention64'),
    ('attention', 32, 64, 768, 12, True, True, 'attention_kernel<64>'),
    ('attn_block', (128, 16, 16, 256), 2, True),
    ('attn_block', (256, 16, 16, 256), 2, True),
    ('attn_block', (32, 16, 16, 256), 2, True),
    ('attn_block', (32, 16, 16, 256), 4, True),
    ('block_stats', (100, 16, 16, 576), 1),
    ('block_stats', (100, 32, 32, 384), 4),
    ('block_stats', (100, 64, 64, 192), 16),
    ('block_stats', (14, 16, 16, 576), 1),
    ('block_stats', (14, 32, 32, 384), 4),
    ('block_stats', (14, 64, 64, 192), 16),
    ('block_stats', (16, 16, 16, 1024), 1),
    ('block_stats', (16, 16, 16, 576), 1),
    ('block_stats', (16, 256, 256, 256), 256),
    ('block_stats', (16, 32, 32, 384), 4),
    ('block_stats', (16, 32, 32, 512), 4),
    ('block_stats', (16, 64, 64, 192), 16),
    ('block_stats', (32, 16, 16, 576), 1),
    ('block_stats', (32, 32, 32, 384), 4),
    ('block_stats', (32, 64, 64, 192), 16),
    ('cm_stage', 0, 0, False, (100, 3, 64, 64), ('x_in', 't')),
    ('cm_stage', 0, 0, False, (14, 3, 64, 64), ('x_in', 't')),
    ('cm_stage', 1, 0, False, (100, 3, 64, 64), ('model_out', 'noise', 'x_in', 't')),
    ('cm_stage', 1, 0, True, (100, 3, 64, 64), ('model_out', 'noise', 'out')),
    ('cm_stage', 1, 1, False, (14, 3, 64, 64), ('model_out', 'noise', 'ref', 'mask', 'x_in', 't')),
    ('cm_stage', 1, 1, True, (14, 3, 64, 64), ('model_out', 'noise', 'ref', 'mask', 'out')),
    ('conv2d', (100, 16, 16, 1152), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (100, 16, 16, 1344), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (100, 16, 16, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (100, 16, 16, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (100, 16, 16, 384), 0, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550060),
    ('conv2d', (100, 16, 16, 384), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (100, 16, 16, 576), 0, 1728, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550090),
    ('conv2d', (100, 16, 16, 576), 0, 576, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 550091),
    ('conv2d', (100, 16, 16, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (100, 16, 16, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (100, 16, 16, 576), 0, 576, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (100, 16, 16, 576), 384, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (100, 16, 16, 576), 576, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (100, 16, 16, 768), 0, 768, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (100, 16, 16, 768), 576, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (100, 16, 16, 960), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (100, 3, 64, 64), 0, 192, 3, True, 1, 1, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 300000),
    ('conv2d', (100, 32, 32, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (100, 32, 32, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (100, 32, 32, 192), 0, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (100, 32, 32, 192), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (100, 32, 32, 384), 0, 1152, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 503030),
    ('conv2d', (100, 32, 32, 384), 0, 384, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 503031),
    ('conv2d', (100, 32, 32, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (100, 32, 32, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (100, 32, 32, 384), 0, 384, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (100, 32, 32, 384), 192, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550090),
    ('conv2d', (100, 32, 32, 384), 384, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (100, 32, 32, 576), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (100, 32, 32, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (100, 32, 32, 576), 384, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (100, 32, 32, 768), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (100, 32, 32, 960), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (100, 64, 64, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (100, 64, 64, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (100, 64, 64, 192), 0, 3, 3, False, 1, 1, None, 0, True, '-', False, False, 0, True, False, None, 0, 0, 'default', 1206),
    ('conv2d', (100, 64, 64, 192), 192, 192, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550060),
    ('conv2d', (100, 64, 64, 384), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (100, 64, 64, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (100, 64, 64, 384), 192, 192, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550090),
    ('conv2d', (100, 64, 64, 576), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (100, 8, 8, 1344), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (100, 8, 8, 1536), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (100, 8, 8, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (100, 8, 8, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (100, 8, 8, 576), 0, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (100, 8, 8, 576), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (100, 8, 8, 768), 0, 2304, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (100, 8, 8, 768), 0, 768, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (100, 8, 8, 768), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (100, 8, 8, 768), 0, 768, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (100, 8, 8, 768), 0, 768, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (100, 8, 8, 768), 576, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (100, 8, 8, 768), 768, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (128, 16, 16, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (128, 16, 16, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (128, 16, 16, 128), 0, 256, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 501030),
    ('conv2d', (128, 16, 16, 128), 0, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 501030),
    ('conv2d', (128, 16, 16, 128), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (128, 16, 16, 128), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (128, 16, 16, 128), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (128, 16, 16, 256), 0, 256, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 502031),
    ('conv2d', (128, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (128, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (128, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (128, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (128, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (128, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (128, 16, 16, 256), 0, 256, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (128, 16, 16, 256), 0, 256, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 30206),
    ('conv2d', (128, 16, 16, 256), 0, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 502030),
    ('conv2d', (128, 16, 16, 256), 128, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 503030),
    ('conv2d', (128, 16, 16, 256), 256, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 504060),
    ('conv2d', (128, 16, 16, 384), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (128, 16, 16, 384), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (128, 16, 16, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (128, 16, 16, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (128, 3, 32, 32), 0, 128, 3, True, 1, 1, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 300000),
    ('conv2d', (128, 3, 32, 32), 0, 128, 3, True, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 300000),
    ('conv2d', (128, 3, 32, 32), 0, 128, 3, True, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 300000),
    ('conv2d', (128, 32, 32, 128), 0, 128, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 501030),
    ('conv2d', (128, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (128, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (128, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (128, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (128, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (128, 32, 32, 128), 0, 128, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (128, 32, 32, 128), 0, 128, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, True, None, 0, 4, 'default', 30206),
    ('conv2d', (128, 32, 32, 128), 0, 3, 3, False, 1, 1, None, 0, True, '-', False, False, 0, True, False, None, 0, 0, 'default', 600000),
    ('conv2d', (128, 32, 32, 128), 128, 128, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 502030),
    ('conv2d', (128, 32, 32, 256), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (128, 32, 32, 256), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (128, 32, 32, 256), 128, 128, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 503030),
    ('conv2d', (128, 32, 32, 384), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (128, 32, 32, 384), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (128, 4, 4, 256), 0, 256, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (128, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 450432),
    ('conv2d', (128, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, (32, False, True, True), 0, 0, 'default', 450432),
    ('conv2d', (128, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, (32, True, True, True), 0, 0, 'default', 450432),
    ('conv2d', (128, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 450432),
    ('conv2d', (128, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 450432),
    ('conv2d', (128, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, (32, True, False, True), 0, 0, 'default', 450432),
    ('conv2d', (128, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 450432),
    ('conv2d', (128, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 400008),
    ('conv2d', (128, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (128, 4, 4, 256), 0, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (128, 4, 4, 256), 256, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (128, 4, 4, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, (32, True, False, True), 0, 0, 'default', 450432),
    ('conv2d', (128, 4, 4, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 450432),
    ('conv2d', (128, 8, 8, 256), 0, 256, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (128, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 450864),
    ('conv2d', (128, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, (32, True, True, False), 0, 0, 'default', 400008),
    ('conv2d', (128, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, (32, True, True, False), 0, 0, 'throughput', 450864),
    ('conv2d', (128, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 400008),
    ('conv2d', (128, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 450864),
    ('conv2d', (128, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 450864),
    ('conv2d', (128, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, (32, True, False, False), 0, 0, 'throughput', 450864),
    ('conv2d', (128, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, (32, True, False, True), 0, 0, 'default', 400008),
    ('conv2d', (128, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 450864),
    ('conv2d', (128, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (128, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (128, 8, 8, 256), 0, 256, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (128, 8, 8, 256), 0, 256, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 30206),
    ('conv2d', (128, 8, 8, 256), 256, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (128, 8, 8, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, (32, True, False, False), 0, 0, 'throughput', 450864),
    ('conv2d', (128, 8, 8, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, (32, True, False, True), 0, 0, 'default', 400008),
    ('conv2d', (128, 8, 8, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 450864),
    ('conv2d', (14, 16, 16, 1152), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (14, 16, 16, 1344), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (14, 16, 16, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (14, 16, 16, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (14, 16, 16, 384), 0, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (14, 16, 16, 384), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (14, 16, 16, 576), 0, 1728, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (14, 16, 16, 576), 0, 576, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (14, 16, 16, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (14, 16, 16, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (14, 16, 16, 576), 0, 576, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (14, 16, 16, 576), 384, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (14, 16, 16, 576), 576, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (14, 16, 16, 768), 0, 768, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (14, 16, 16, 768), 576, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (14, 16, 16, 960), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (14, 3, 64, 64), 0, 192, 3, True, 1, 1, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 300000),
    ('conv2d', (14, 32, 32, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (14, 32, 32, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (14, 32, 32, 192), 0, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (14, 32, 32, 192), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (14, 32, 32, 384), 0, 1152, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550060),
    ('conv2d', (14, 32, 32, 384), 0, 384, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (14, 32, 32, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (14, 32, 32, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (14, 32, 32, 384), 0, 384, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (14, 32, 32, 384), 192, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (14, 32, 32, 384), 384, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (14, 32, 32, 576), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (14, 32, 32, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (14, 32, 32, 576), 384, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (14, 32, 32, 768), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (14, 32, 32, 960), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (14, 64, 64, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (14, 64, 64, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (14, 64, 64, 192), 0, 3, 3, False, 1, 1, None, 0, True, '-', False, False, 0, True, False, None, 0, 0, 'default', 1206),
    ('conv2d', (14, 64, 64, 192), 192, 192, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550060),
    ('conv2d', (14, 64, 64, 384), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (14, 64, 64, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (14, 64, 64, 384), 192, 192, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550090),
    ('conv2d', (14, 64, 64, 576), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (14, 8, 8, 1344), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (14, 8, 8, 1536), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (14, 8, 8, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (14, 8, 8, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (14, 8, 8, 576), 0, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (14, 8, 8, 576), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (14, 8, 8, 768), 0, 2304, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (14, 8, 8, 768), 0, 768, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (14, 8, 8, 768), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (14, 8, 8, 768), 0, 768, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (14, 8, 8, 768), 0, 768, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (14, 8, 8, 768), 576, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (14, 8, 8, 768), 768, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 128, 128, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 4, 'default', 400032),
    ('conv2d', (16, 128, 128, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 4, 'default', 400032),
    ('conv2d', (16, 128, 128, 256), 0, 256, 3, False, 1, 1, None, 1, True, 'image', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 128, 128, 256), 256, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 504060),
    ('conv2d', (16, 128, 128, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 4, 'default', 400032),
    ('conv2d', (16, 128, 128, 512), 0, 512, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 4, 'default', 400032),
    ('conv2d', (16, 128, 128, 512), 256, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 128, 128, 768), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 4, 'default', 400032),
    ('conv2d', (16, 16, 16, 1024), 0, 1024, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 16, 16, 1024), 0, 1024, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 16, 16, 1024), 0, 1024, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 16, 16, 1024), 0, 1024, 3, False, 1, 1, None, 1, True, 'image', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (16, 16, 16, 1024), 0, 3072, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 16, 16, 1024), 1024, 1024, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 16, 16, 1024), 512, 1024, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 16, 16, 1152), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'throughput', 30206),
    ('conv2d', (16, 16, 16, 1152), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 16, 16, 1344), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'throughput', 30206),
    ('conv2d', (16, 16, 16, 1344), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 16, 16, 1536), 0, 1024, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 16, 16, 2048), 0, 1024, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 16, 16, 256), 0, 256, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (16, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (16, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (16, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (16, 16, 16, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 16, 16, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 4, 'throughput', 30206),
    ('conv2d', (16, 16, 16, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 16, 16, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 4, 'throughput', 30206),
    ('conv2d', (16, 16, 16, 384), 0, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 16, 16, 384), 0, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (16, 16, 16, 384), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'throughput', 30206),
    ('conv2d', (16, 16, 16, 384), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 16, 16, 512), 0, 1024, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 16, 16, 512), 0, 1024, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 16, 16, 512), 0, 512, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 16, 16, 512), 0, 512, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 16, 16, 576), 0, 1728, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550090),
    ('conv2d', (16, 16, 16, 576), 0, 1728, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 550090),
    ('conv2d', (16, 16, 16, 576), 0, 576, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 16, 16, 576), 0, 576, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (16, 16, 16, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'throughput', 30206),
    ('conv2d', (16, 16, 16, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 16, 16, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 0, 'throughput', 30206),
    ('conv2d', (16, 16, 16, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 16, 16, 576), 0, 576, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (16, 16, 16, 576), 0, 576, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 8, 'throughput', 400032),
    ('conv2d', (16, 16, 16, 576), 384, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 16, 16, 576), 384, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (16, 16, 16, 576), 576, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 16, 16, 576), 576, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (16, 16, 16, 768), 0, 768, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 16, 16, 768), 0, 768, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'throughput', 400016),
    ('conv2d', (16, 16, 16, 768), 576, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 16, 16, 768), 576, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (16, 16, 16, 960), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'throughput', 30206),
    ('conv2d', (16, 16, 16, 960), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 256, 256, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 256, 256, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 256, 256, 256), 0, 3, 3, False, 1, 1, None, 0, True, '-', False, False, 0, True, False, None, 0, 0, 'default', 1206),
    ('conv2d', (16, 256, 256, 256), 256, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 504060),
    ('conv2d', (16, 256, 256, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 3, 256, 256), 0, 256, 3, True, 1, 1, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 300000),
    ('conv2d', (16, 3, 64, 64), 0, 128, 3, True, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 300000),
    ('conv2d', (16, 3, 64, 64), 0, 192, 3, True, 1, 1, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 300000),
    ('conv2d', (16, 3, 64, 64), 0, 192, 3, True, 1, 1, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 300000),
    ('conv2d', (16, 32, 32, 1024), 0, 1024, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (16, 32, 32, 1024), 0, 512, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (16, 32, 32, 1024), 512, 512, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (16, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (16, 32, 32, 128), 0, 256, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (16, 32, 32, 128), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (16, 32, 32, 1536), 0, 512, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (16, 32, 32, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (16, 32, 32, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'throughput', 400032),
    ('conv2d', (16, 32, 32, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (16, 32, 32, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'throughput', 400032),
    ('conv2d', (16, 32, 32, 192), 0, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 32, 32, 192), 0, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (16, 32, 32, 192), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (16, 32, 32, 192), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'throughput', 400032),
    ('conv2d', (16, 32, 32, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (16, 32, 32, 384), 0, 1152, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550060),
    ('conv2d', (16, 32, 32, 384), 0, 1152, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 550060),
    ('conv2d', (16, 32, 32, 384), 0, 384, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 550061),
    ('conv2d', (16, 32, 32, 384), 0, 384, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 550061),
    ('conv2d', (16, 32, 32, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (16, 32, 32, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'throughput', 400032),
    ('conv2d', (16, 32, 32, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (16, 32, 32, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'throughput', 400032),
    ('conv2d', (16, 32, 32, 384), 0, 384, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 32, 32, 384), 0, 384, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 1, 'throughput', 400032),
    ('conv2d', (16, 32, 32, 384), 192, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550090),
    ('conv2d', (16, 32, 32, 384), 192, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 550090),
    ('conv2d', (16, 32, 32, 384), 384, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 32, 32, 384), 384, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (16, 32, 32, 512), 0, 1536, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550080),
    ('conv2d', (16, 32, 32, 512), 0, 512, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 550081),
    ('conv2d', (16, 32, 32, 512), 0, 512, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (16, 32, 32, 512), 0, 512, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (16, 32, 32, 512), 0, 512, 3, False, 1, 1, None, 1, True, 'image', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 32, 32, 512), 512, 512, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 32, 32, 576), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (16, 32, 32, 576), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'throughput', 400032),
    ('conv2d', (16, 32, 32, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (16, 32, 32, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'throughput', 400032),
    ('conv2d', (16, 32, 32, 576), 384, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 32, 32, 576), 384, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (16, 32, 32, 768), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (16, 32, 32, 768), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'throughput', 400032),
    ('conv2d', (16, 32, 32, 960), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (16, 32, 32, 960), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'throughput', 400032),
    ('conv2d', (16, 64, 64, 1024), 0, 512, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 64, 64, 128), 0, 128, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 501030),
    ('conv2d', (16, 64, 64, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (16, 64, 64, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (16, 64, 64, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 64, 64, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'throughput', 400032),
    ('conv2d', (16, 64, 64, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 64, 64, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 1, 'throughput', 400032),
    ('conv2d', (16, 64, 64, 192), 0, 3, 3, False, 1, 1, None, 0, True, '-', False, False, 0, True, False, None, 0, 0, 'default', 1206),
    ('conv2d', (16, 64, 64, 192), 0, 3, 3, False, 1, 1, None, 0, True, '-', False, False, 0, True, False, None, 0, 0, 'throughput', 1206),
    ('conv2d', (16, 64, 64, 192), 192, 192, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550060),
    ('conv2d', (16, 64, 64, 192), 192, 192, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 550060),
    ('conv2d', (16, 64, 64, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 64, 64, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 64, 64, 256), 0, 512, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 502030),
    ('conv2d', (16, 64, 64, 256), 0, 512, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 64, 64, 384), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 64, 64, 384), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'throughput', 400032),
    ('conv2d', (16, 64, 64, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 64, 64, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 1, 'throughput', 400032),
    ('conv2d', (16, 64, 64, 384), 192, 192, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550090),
    ('conv2d', (16, 64, 64, 384), 192, 192, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 550090),
    ('conv2d', (16, 64, 64, 512), 0, 512, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 64, 64, 512), 0, 512, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 64, 64, 512), 0, 512, 3, False, 1, 1, None, 1, True, 'image', False, False, 0, False, True, None, 0, 4, 'default', 400032),
    ('conv2d', (16, 64, 64, 512), 256, 512, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 64, 64, 512), 512, 512, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 64, 64, 576), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 64, 64, 576), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'throughput', 400032),
    ('conv2d', (16, 64, 64, 768), 0, 512, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (16, 8, 8, 1024), 0, 1024, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 8, 8, 1024), 0, 1024, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 0, 'default', 450832),
    ('conv2d', (16, 8, 8, 1024), 0, 1024, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 0, 'default', 450832),
    ('conv2d', (16, 8, 8, 1024), 0, 1024, 3, False, 1, 1, None, 1, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 8, 8, 1024), 0, 3072, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 8, 8, 1024), 1024, 1024, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 8, 8, 1344), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (16, 8, 8, 1344), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'throughput', 450832),
    ('conv2d', (16, 8, 8, 1536), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (16, 8, 8, 1536), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'throughput', 450832),
    ('conv2d', (16, 8, 8, 2048), 0, 1024, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 0, 'default', 450832),
    ('conv2d', (16, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 450832),
    ('conv2d', (16, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 450832),
    ('conv2d', (16, 8, 8, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (16, 8, 8, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'throughput', 450832),
    ('conv2d', (16, 8, 8, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (16, 8, 8, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 0, 'throughput', 450832),
    ('conv2d', (16, 8, 8, 576), 0, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 8, 8, 576), 0, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (16, 8, 8, 576), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (16, 8, 8, 576), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'throughput', 450832),
    ('conv2d', (16, 8, 8, 768), 0, 2304, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 8, 8, 768), 0, 2304, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (16, 8, 8, 768), 0, 768, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 8, 8, 768), 0, 768, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (16, 8, 8, 768), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (16, 8, 8, 768), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'throughput', 450832),
    ('conv2d', (16, 8, 8, 768), 0, 768, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (16, 8, 8, 768), 0, 768, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 0, 'throughput', 450832),
    ('conv2d', (16, 8, 8, 768), 0, 768, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (16, 8, 8, 768), 0, 768, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 2, 'throughput', 400016),
    ('conv2d', (16, 8, 8, 768), 576, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 8, 8, 768), 576, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (16, 8, 8, 768), 768, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (16, 8, 8, 768), 768, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (256, 16, 16, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (256, 16, 16, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (256, 16, 16, 128), 0, 256, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 501030),
    ('conv2d', (256, 16, 16, 128), 0, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 501030),
    ('conv2d', (256, 16, 16, 128), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (256, 16, 16, 128), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (256, 16, 16, 128), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (256, 16, 16, 256), 0, 256, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 502031),
    ('conv2d', (256, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (256, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (256, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (256, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (256, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (256, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (256, 16, 16, 256), 0, 256, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (256, 16, 16, 256), 0, 256, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 30206),
    ('conv2d', (256, 16, 16, 256), 0, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 502030),
    ('conv2d', (256, 16, 16, 256), 128, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 503030),
    ('conv2d', (256, 16, 16, 256), 256, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 504060),
    ('conv2d', (256, 16, 16, 384), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (256, 16, 16, 384), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (256, 16, 16, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (256, 16, 16, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (256, 3, 32, 32), 0, 128, 3, True, 1, 1, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 300000),
    ('conv2d', (256, 3, 32, 32), 0, 128, 3, True, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 300000),
    ('conv2d', (256, 3, 32, 32), 0, 128, 3, True, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 300000),
    ('conv2d', (256, 32, 32, 128), 0, 128, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 501030),
    ('conv2d', (256, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (256, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (256, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (256, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (256, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (256, 32, 32, 128), 0, 128, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (256, 32, 32, 128), 0, 128, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, True, None, 0, 4, 'default', 30206),
    ('conv2d', (256, 32, 32, 128), 0, 3, 3, False, 1, 1, None, 0, True, '-', False, False, 0, True, False, None, 0, 0, 'default', 600000),
    ('conv2d', (256, 32, 32, 128), 128, 128, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 502030),
    ('conv2d', (256, 32, 32, 256), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (256, 32, 32, 256), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (256, 32, 32, 256), 128, 128, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 503030),
    ('conv2d', (256, 32, 32, 384), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (256, 32, 32, 384), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (256, 4, 4, 256), 0, 256, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (256, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 450432),
    ('conv2d', (256, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, (32, False, True, True), 0, 0, 'default', 450432),
    ('conv2d', (256, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, (32, True, True, True), 0, 0, 'default', 450432),
    ('conv2d', (256, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 450432),
    ('conv2d', (256, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 450432),
    ('conv2d', (256, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, (32, True, False, True), 0, 0, 'default', 450432),
    ('conv2d', (256, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 450432),
    ('conv2d', (256, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 400008),
    ('conv2d', (256, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (256, 4, 4, 256), 0, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (256, 4, 4, 256), 256, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (256, 4, 4, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, (32, True, False, True), 0, 0, 'default', 450432),
    ('conv2d', (256, 4, 4, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 450432),
    ('conv2d', (256, 8, 8, 256), 0, 256, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (256, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400008),
    ('conv2d', (256, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, (32, True, True, False), 0, 0, 'default', 400008),
    ('conv2d', (256, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 400008),
    ('conv2d', (256, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 400008),
    ('conv2d', (256, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, (32, True, False, True), 0, 0, 'default', 400008),
    ('conv2d', (256, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400008),
    ('conv2d', (256, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (256, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (256, 8, 8, 256), 0, 256, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (256, 8, 8, 256), 0, 256, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 30206),
    ('conv2d', (256, 8, 8, 256), 256, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (256, 8, 8, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, (32, True, False, True), 0, 0, 'default', 400008),
    ('conv2d', (256, 8, 8, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400008),
    ('conv2d', (32, 16, 16, 1152), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (32, 16, 16, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (32, 16, 16, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (32, 16, 16, 128), 0, 256, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (32, 16, 16, 128), 0, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 16, 16, 128), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (32, 16, 16, 128), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (32, 16, 16, 128), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (32, 16, 16, 128), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 4, 'throughput', 30206),
    ('conv2d', (32, 16, 16, 1344), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (32, 16, 16, 256), 0, 256, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (32, 16, 16, 256), 0, 256, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (32, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (32, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (32, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (32, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 4, 'throughput', 30206),
    ('conv2d', (32, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (32, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (32, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (32, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 4, 'throughput', 30206),
    ('conv2d', (32, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (32, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (32, 16, 16, 256), 0, 256, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (32, 16, 16, 256), 0, 256, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 30206),
    ('conv2d', (32, 16, 16, 256), 0, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (32, 16, 16, 256), 128, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 16, 16, 256), 256, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 16, 16, 384), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (32, 16, 16, 384), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (32, 16, 16, 384), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 4, 'throughput', 30206),
    ('conv2d', (32, 16, 16, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (32, 16, 16, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (32, 16, 16, 384), 0, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 16, 16, 384), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (32, 16, 16, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (32, 16, 16, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (32, 16, 16, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 4, 'throughput', 30206),
    ('conv2d', (32, 16, 16, 576), 0, 1728, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550090),
    ('conv2d', (32, 16, 16, 576), 0, 576, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 16, 16, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (32, 16, 16, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (32, 16, 16, 576), 0, 576, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (32, 16, 16, 576), 384, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 16, 16, 576), 576, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 16, 16, 768), 0, 768, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (32, 16, 16, 768), 576, 576, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 16, 16, 960), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (32, 3, 32, 32), 0, 128, 3, True, 1, 1, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 300000),
    ('conv2d', (32, 3, 32, 32), 0, 128, 3, True, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 300000),
    ('conv2d', (32, 3, 32, 32), 0, 128, 3, True, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 300000),
    ('conv2d', (32, 3, 64, 64), 0, 128, 3, True, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 300000),
    ('conv2d', (32, 3, 64, 64), 0, 192, 3, True, 1, 1, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 300000),
    ('conv2d', (32, 32, 32, 128), 0, 128, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 501030),
    ('conv2d', (32, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (32, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (32, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (32, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (32, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (32, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (32, 32, 32, 128), 0, 128, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (32, 32, 32, 128), 0, 128, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, True, None, 0, 4, 'default', 30206),
    ('conv2d', (32, 32, 32, 128), 0, 256, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 501030),
    ('conv2d', (32, 32, 32, 128), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (32, 32, 32, 128), 0, 3, 3, False, 1, 1, None, 0, True, '-', False, False, 0, True, False, None, 0, 0, 'default', 600000),
    ('conv2d', (32, 32, 32, 128), 128, 128, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 502030),
    ('conv2d', (32, 32, 32, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (32, 32, 32, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (32, 32, 32, 192), 0, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 32, 32, 192), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (32, 32, 32, 256), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (32, 32, 32, 256), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (32, 32, 32, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (32, 32, 32, 256), 128, 128, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 503030),
    ('conv2d', (32, 32, 32, 384), 0, 1152, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 503030),
    ('conv2d', (32, 32, 32, 384), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (32, 32, 32, 384), 0, 128, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (32, 32, 32, 384), 0, 384, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 503031),
    ('conv2d', (32, 32, 32, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (32, 32, 32, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (32, 32, 32, 384), 0, 384, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (32, 32, 32, 384), 192, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550090),
    ('conv2d', (32, 32, 32, 384), 384, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 32, 32, 576), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (32, 32, 32, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (32, 32, 32, 576), 384, 384, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 32, 32, 768), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (32, 32, 32, 960), 0, 384, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 8, 'default', 400032),
    ('conv2d', (32, 4, 4, 256), 0, 256, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 450432),
    ('conv2d', (32, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, (32, False, True, True), 0, 0, 'default', 450432),
    ('conv2d', (32, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, (32, True, True, True), 0, 0, 'default', 450432),
    ('conv2d', (32, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 450432),
    ('conv2d', (32, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 450432),
    ('conv2d', (32, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, (32, True, False, True), 0, 0, 'default', 450432),
    ('conv2d', (32, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 450432),
    ('conv2d', (32, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 400008),
    ('conv2d', (32, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (32, 4, 4, 256), 0, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 4, 4, 256), 256, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 4, 4, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, (32, True, False, True), 0, 0, 'default', 450432),
    ('conv2d', (32, 4, 4, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 450432),
    ('conv2d', (32, 64, 64, 128), 0, 128, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 501030),
    ('conv2d', (32, 64, 64, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (32, 64, 64, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (32, 64, 64, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (32, 64, 64, 192), 0, 192, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (32, 64, 64, 192), 0, 3, 3, False, 1, 1, None, 0, True, '-', False, False, 0, True, False, None, 0, 0, 'default', 1206),
    ('conv2d', (32, 64, 64, 192), 192, 192, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550060),
    ('conv2d', (32, 64, 64, 384), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (32, 64, 64, 384), 0, 384, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (32, 64, 64, 384), 192, 192, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 550090),
    ('conv2d', (32, 64, 64, 576), 0, 192, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 1, 'default', 400032),
    ('conv2d', (32, 8, 8, 1344), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (32, 8, 8, 1536), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (32, 8, 8, 256), 0, 256, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (32, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 450832),
    ('conv2d', (32, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, (32, True, True, False), 0, 0, 'default', 400008),
    ('conv2d', (32, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, (32, True, True, False), 0, 0, 'throughput', 450832),
    ('conv2d', (32, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 400008),
    ('conv2d', (32, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 450832),
    ('conv2d', (32, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 450832),
    ('conv2d', (32, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, (32, True, False, False), 0, 0, 'throughput', 450832),
    ('conv2d', (32, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, (32, True, False, True), 0, 0, 'default', 400008),
    ('conv2d', (32, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 450832),
    ('conv2d', (32, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (32, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (32, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 4, 'throughput', 30206),
    ('conv2d', (32, 8, 8, 256), 0, 256, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (32, 8, 8, 256), 0, 256, 3, False, 2, 0, 1, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 30206),
    ('conv2d', (32, 8, 8, 256), 256, 256, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 8, 8, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, (32, True, False, False), 0, 0, 'throughput', 450832),
    ('conv2d', (32, 8, 8, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, (32, True, False, True), 0, 0, 'default', 400008),
    ('conv2d', (32, 8, 8, 512), 0, 256, 3, False, 1, 1, None, 0, True, 'image', False, False, 0, False, False, None, 0, 0, 'throughput', 450832),
    ('conv2d', (32, 8, 8, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (32, 8, 8, 576), 0, 576, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (32, 8, 8, 576), 0, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 8, 8, 576), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (32, 8, 8, 768), 0, 2304, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 8, 8, 768), 0, 768, 1, False, 1, 0, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 8, 8, 768), 0, 768, 3, False, 1, 1, None, 0, True, '-', False, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (32, 8, 8, 768), 0, 768, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, True, None, 0, 0, 'default', 400008),
    ('conv2d', (32, 8, 8, 768), 0, 768, 3, False, 1, 1, None, 1, True, '-', False, False, 0, False, True, None, 0, 2, 'default', 400016),
    ('conv2d', (32, 8, 8, 768), 576, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (32, 8, 8, 768), 768, 768, 1, False, 1, 0, None, 0, True, '-', False, False, 0, False, False, None, 0, 0, 'default', 200000),
    ('conv2d', (512, 16, 16, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (512, 16, 16, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (512, 16, 16, 128), 0, 256, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 501030),
    ('conv2d', (512, 16, 16, 128), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (512, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (512, 3, 32, 32), 0, 128, 3, True, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 300000),
    ('conv2d', (512, 32, 32, 128), 0, 128, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 501030),
    ('conv2d', (512, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (512, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (512, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 450464),
    ('conv2d', (512, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 450464),
    ('conv2d', (512, 8, 8, 256), 0, 256, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 502030),
    ('conv2d', (512, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400008),
    ('conv2d', (512, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 400008),
    ('conv2d', (512, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 400008),
    ('conv2d', (64, 16, 16, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (64, 16, 16, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 30206),
    ('conv2d', (64, 16, 16, 128), 0, 256, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (64, 16, 16, 128), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (64, 16, 16, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 400016),
    ('conv2d', (64, 3, 32, 32), 0, 128, 3, True, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 300000),
    ('conv2d', (64, 32, 32, 128), 0, 128, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 501030),
    ('conv2d', (64, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (64, 32, 32, 128), 0, 128, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 400032),
    ('conv2d', (64, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 450432),
    ('conv2d', (64, 4, 4, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 450432),
    ('conv2d', (64, 8, 8, 256), 0, 256, 1, False, 1, 0, None, 0, False, '-', False, False, 0, False, False, None, 0, 0, 'throughput', 200000),
    ('conv2d', (64, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', False, False, 1, False, False, None, 0, 0, 'throughput', 450832),
    ('conv2d', (64, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 0, False, False, None, 0, 0, 'throughput', 450832),
    ('conv2d', (64, 8, 8, 256), 0, 256, 3, False, 1, 1, None, 0, True, '-', True, False, 1, False, False, None, 0, 0, 'throughput', 450832),
    ('dropout', (128, 16, 16, 256), 0.1, False),
    ('dropout', (128, 32, 32, 128), 0.1, False),
    ('dropout', (128, 4, 4, 256), 0.1, False),
    ('dropout', (128, 8, 8, 256), 0.1, False),
    ('dropout', (16, 16, 16, 384), 0.1, False),
    ('dropout', (16, 16, 16, 576), 0.1, False),
    ('dropout', (16, 16, 16, 768), 0.1, False),
    ('dropout', (16, 32, 32, 192), 0.1, False),
    ('dropout', (16, 32, 32, 384), 0.1, False),
    ('dropout', (16, 32, 32, 576), 0.1, False),
    ('dropout', (16, 64, 64, 192), 0.1, False),
    ('dropout', (16, 64, 64, 384), 0.1, False),
    ('dropout', (16, 8, 8, 576), 0.1, False),
    ('dropout', (16, 8, 8, 768), 0.1, False),
    ('dropout', (256, 16, 16, 256), 0.1, False),
    ('dropout', (256, 32, 32, 128), 0.1, False),
    ('dropout', (256, 4, 4, 256), 0.1, False),
    ('dropout', (256, 8, 8, 256), 0.1, False),
    ('dropout', (32, 16, 16, 256), 0.1, False),
    ('dropout', (32, 16, 16, 384), 0.1, False),
    ('dropout', (32, 16, 16, 576), 0.1, False),
    ('dropout', (32, 16, 16, 768), 0.1, False),
    ('dropout', (32, 32, 32, 128), 0.1, False),
    ('dropout', (32, 32, 32, 192), 0.1, False),
    ('dropout', (32, 32, 32, 384), 0.1, False),
    ('dropout', (32, 32, 32, 576), 0.1, False),
    ('dropout', (32, 4, 4, 256), 0.1, False),
    ('dropout', (32, 64, 64, 192), 0.1, False),
    ('dropout', (32, 64, 64, 384), 0.1, False),
    ('dropout', (32, 8, 8, 256), 0.1, False),
    ('dropout', (32, 8, 8, 576), 0.1, False),
    ('dropout', (32, 8, 8, 768), 0.1, False),
    ('edm_dsm_loss_fwd', (16, 3, 64, 64), 'karras', False),
    ('edm_dsm_loss_fwd', (32, 3, 64, 64), 'karras', False),
    ('edm_dsm_prep', (16, 3, 64, 64)),
    ('edm_dsm_prep', (32, 3, 64, 64)),
    ('edm_precond', (100, 3, 64, 64)),
    ('edm_precond', (16, 3, 256, 256)),
    ('edm_precond', (16, 3, 64, 64)),
    ('edm_step', (100, 3, 64, 64)),
    ('edm_step', (16, 3, 256, 256)),
    ('edm_step', (16, 3, 64, 64)),
    ('fold_stats', 100, 16, 192, 32),
    ('fold_stats', 100, 32, 192, 32),
    ('fold_stats', 100, 32, 384, 32),
    ('fold_stats', 14, 16, 192, 32),
    ('fold_stats', 14, 32, 192, 32),
    ('fold_stats', 14, 32, 384, 32),
    ('fold_stats', 16, 128, 256, 32),
    ('fold_stats', 16, 128, 512, 32),
    ('fold_stats', 16, 16, 192, 32),
    ('fold_stats', 16, 256, 256, 32),
    ('fold_stats', 16, 32, 192, 32),
    ('fold_stats', 16, 32, 256, 32),
    ('fold_stats', 16, 32, 384, 32),
    ('fold_stats', 16, 32, 512, 32),
    ('fold_stats', 16, 512, 256, 32),
    ('fold_stats', 32, 16, 192, 32),
    ('fold_stats', 32, 32, 192, 32),
    ('fold_stats', 32, 32, 384, 32),
    ('gn', 'apply', (100, 16, 16, 384), 0, 32, 1e-05, True, False, False, 2, 0),
    ('gn', 'apply', (100, 16, 16, 384), 0, 32, 1e-05, True, True, False, 2, 0),
    ('gn', 'apply', (100, 16, 16, 576), 0, 32, 1e-05, False, False, False, 2, 0),
    ('gn', 'apply', (100, 16, 16, 576), 0, 32, 1e-05, True, False, False, 1, 0),
    ('gn', 'apply', (100, 16, 16, 576), 0, 32, 1e-05, True, True, False, 2, 0),
    ('gn', 'apply', (100, 16, 16, 576), 384, 32, 1e-05, True, False, False, 1, 2),
    ('gn', 'apply', (100, 16, 16, 576), 576, 32, 1e-05, True, False, False, 1, 1),
    ('gn', 'apply', (100, 16, 16, 768), 0, 32, 1e-05, True, True, False, 2, 0),
    ('gn', 'apply', (100, 16, 16, 768), 576, 32, 1e-05, True, False, False, 2, 1),
    ('gn', 'apply', (100, 32, 32, 192), 0, 32, 1e-05, True, False, False, 8, 0),
    ('gn', 'apply', (100, 32, 32, 192), 0, 32, 1e-05, True, True, False, 8, 0),
    ('gn', 'apply', (100, 32, 32, 384), 0, 32, 1e-05, False, False, False, 8, 0),
    ('gn', 'apply', (100, 32, 32, 384), 0, 32, 1e-05, True, False, False, 4, 0),
    ('gn', 'apply', (100, 32, 32, 384), 0, 32, 1e-05, True, True, False, 8, 0),
    ('gn', 'apply', (100, 32, 32, 384), 192, 32, 1e-05, True, False, False, 4, 8),
    ('gn', 'apply', (100, 32, 32, 384), 384, 32, 1e-05, True, False, False, 4, 4),
    ('gn', 'apply', (100, 32, 32, 576), 0, 32, 1e-05, True, True, False, 8, 0),
    ('gn', 'apply', (100, 32, 32, 576), 384, 32, 1e-05, True, False, False, 8, 4),
    ('gn', 'apply', (100, 64, 64, 192), 0, 32, 1e-05, True, False, False, 1, 0),
    ('gn', 'apply', (100, 64, 64, 192), 0, 32, 1e-05, True, True, False, 1, 0),
    ('gn', 'apply', (100, 64, 64, 192), 192, 32, 1e-05, True, False, False, 1, 1),
    ('gn', 'apply', (100, 64, 64, 384), 0, 32, 1e-05, True, True, False, 1, 0),
    ('gn', 'apply', (100, 64, 64, 384), 192, 32, 1e-05, True, False, False, 1, 1),
    ('gn', 'apply', (128, 16, 16, 128), 0, 32, 1e-06, True, False, False, 4, 0),
    ('gn', 'apply', (128, 16, 16, 256), 0, 32, 1e-06, True, False, False, 2, 0),
    ('gn', 'apply', (128, 16, 16, 256), 0, 32, 1e-06, True, False, False, 8, 0),
    ('gn', 'apply', (128, 16, 16, 256), 128, 32, 1e-06, True, False, False, 8, 4),
    ('gn', 'apply', (128, 16, 16, 256), 256, 32, 1e-06, True, False, False, 2, 8),
    ('gn', 'apply', (128, 16, 16, 256), 256, 32, 1e-06, True, False, False, 8, 8),
    ('gn', 'apply', (128, 32, 32, 128), 0, 32, 1e-06, True, False, False, 8, 0),
    ('gn', 'apply', (128, 32, 32, 128), 128, 32, 1e-06, True, False, False, 8, 8),
    ('gn', 'apply', (128, 32, 32, 256), 128, 32, 1e-06, True, False, False, 8, 8),
    ('gn', 'apply', (128, 8, 8, 256), 0, 32, 1e-06, True, False, False, 1, 0),
    ('gn', 'apply', (14, 16, 16, 384), 0, 32, 1e-05, True, False, False, 2, 0),
    ('gn', 'apply', (14, 16, 16, 384), 0, 32, 1e-05, True, True, False, 2, 0),
    ('gn', 'apply', (14, 16, 16, 576), 0, 32, 1e-05, False, False, False, 2, 0),
    ('gn', 'apply', (14, 16, 16, 576), 0, 32, 1e-05, True, False, False, 1, 0),
    ('gn', 'apply', (14, 16, 16, 576), 0, 32, 1e-05, True, True, False, 2, 0),
    ('gn', 'apply', (14, 16, 16, 576), 384, 32, 1e-05, True, False, False, 1, 2),
    ('gn', 'apply', (14, 16, 16, 576), 576, 32, 1e-05, True, False, False, 1, 1),
    ('gn', 'apply', (14, 16, 16, 768), 0, 32, 1e-05, True, True, False, 2, 0),
    ('gn', 'apply', (14, 16, 16, 768), 576, 32, 1e-05, True, False, False, 2, 1),
    ('gn', 'apply', (14, 32, 32, 192), 0, 32, 1e-05, True, False, False, 8, 0),
    ('gn', 'apply', (14, 32, 32, 192), 0, 32, 1e-05, True, True, False, 8, 0),
    ('gn', 'apply', (14, 32, 32, 384), 0, 32, 1e-05, False, False, False, 8, 0),
    ('gn', 'apply', (14, 32, 32, 384), 0, 32, 1e-05, True, False, False, 4, 0),
    ('gn', 'apply', (14, 32, 32, 384), 0, 32, 1e-05, True, True, False, 8, 0),
    ('gn', 'apply', (14, 32, 32, 384), 192, 32, 1e-05, True, False, False, 4, 8),
    ('gn', 'apply', (14, 32, 32, 384), 384, 32, 1e-05, True, False, False, 4, 4),
    ('gn', 'apply', (14, 32, 32, 576), 0, 32, 1e-05, True, True, False, 8, 0),
    ('gn', 'apply', (14, 32, 32, 576), 384, 32, 1e-05, True, False, False, 8, 4),
    ('gn', 'apply', (14, 64, 64, 192), 0, 32, 1e-05, True, False, False, 1, 0),
    ('gn', 'apply', (14, 64, 64, 192), 0, 32, 1e-05, True, True, False, 1, 0),
    ('gn', 'apply', (14, 64, 64, 192), 192, 32, 1e-05, True, False, False, 1, 1),
    ('gn', 'apply', (14, 64, 64, 384), 0, 32, 1e-05, True, True, False, 1, 0),
    ('gn', 'apply', (14, 64, 64, 384), 192, 32, 1e-05, True, False, False, 1, 1),
    ('gn', 'apply', (16, 128, 128, 256), 0, 32, 1e-05, True, False, False, 4, 0),
    ('gn', 'apply', (16, 128, 128, 256), 256, 32, 1e-05, True, False, False, 4, 4),
    ('gn', 'apply', (16, 128, 128, 512), 0, 32, 1e-05, True, False, False, 4, 0),
    ('gn', 'apply', (16, 128, 128, 512), 256, 32, 1e-05, True, False, False, 4, 4),
    ('gn', 'apply', (16, 16, 16, 1024), 0, 32, 1e-05, False, False, False, 2, 0),
    ('gn', 'apply', (16, 16, 16, 1024), 0, 32, 1e-05, True, False, False, 1, 0),
    ('gn', 'apply', (16, 16, 16, 1024), 0, 32, 1e-05, True, False, False, 2, 0),
    ('gn', 'apply', (16, 16, 16, 1024), 1024, 32, 1e-05, True, False, False, 1, 1),
    ('gn', 'apply', (16, 16, 16, 1024), 1024, 32, 1e-05, True, False, False, 2, 1),
    ('gn', 'apply', (16, 16, 16, 1024), 512, 32, 1e-05, True, False, False, 1, 2),
    ('gn', 'apply', (16, 16, 16, 384), 0, 32, 1e-05, True, False, False, 2, 0),
    ('gn', 'apply', (16, 16, 16, 384), 0, 32, 1e-05, True, False, False, 4, 0),
    ('gn', 'apply', (16, 16, 16, 384), 0, 32, 1e-05, True, True, False, 2, 0),
    ('gn', 'apply', (16, 16, 16, 384), 0, 32, 1e-05, True, True, False, 4, 0),
    ('gn', 'apply', (16, 16, 16, 512), 0, 32, 1e-05, True, False, False, 2, 0),
    ('gn', 'apply', (16, 16, 16, 576), 0, 32, 1e-05, False, False, False, 1, 0),
    ('gn', 'apply', (16, 16, 16, 576), 0, 32, 1e-05, False, False, False, 2, 0),
    ('gn', 'apply', (16, 16, 16, 576), 0, 32, 1e-05, True, False, False, 1, 0),
    ('gn', 'apply', (16, 16, 16, 576), 0, 32, 1e-05, True, True, False, 2, 0),
    ('gn', 'apply', (16, 16, 16, 576), 384, 32, 1e-05, True, False, False, 1, 2),
    ('gn', 'apply', (16, 16, 16, 576), 384, 32, 1e-05, True, False, False, 1, 4),
    ('gn', 'apply', (16, 16, 16, 576), 576, 32, 1e-05, True, False, False, 1, 1),
    ('gn', 'apply', (16, 16, 16, 768), 0, 32, 1e-05, True, True, False, 2, 0),
    ('gn', 'apply', (16, 16, 16, 768), 576, 32, 1e-05, True, False, False, 2, 1),
    ('gn', 'apply', (16, 256, 256, 256), 0, 32, 1e-05, True, False, False, 1, 0),
    ('gn', 'apply', (16, 256, 256, 256), 0, 32, 1e-05, True, False, False, 8, 0),
    ('gn', 'apply', (16, 256, 256, 256), 256, 32, 1e-05, True, False, False, 1, 1),
    ('gn', 'apply', (16, 256, 256, 256), 256, 32, 1e-05, True, False, False, 1, 8),
    ('gn', 'apply', (16, 32, 32, 1024), 0, 32, 1e-05, True, False, False, 8, 0),
    ('gn', 'apply', (16, 32, 32, 1024), 512, 32, 1e-05, True, False, False, 8, 4),
    ('gn', 'apply', (16, 32, 32, 192), 0, 32, 1e-05, True, False, False, 8, 0),
    ('gn', 'apply', (16, 32, 32, 192), 0, 32, 1e-05, True, True, False, 8, 0),
    ('gn', 'apply', (16, 32, 32, 384), 0, 32, 1e-05, False, False, False, 8, 0),
    ('gn', 'apply', (16, 32, 32, 384), 0, 32, 1e-05, True, False, False, 4, 0),
    ('gn', 'apply', (16, 32, 32, 384), 0, 32, 1e-05, True, True, False, 8, 0),
    ('gn', 'apply', (16, 32, 32, 384), 192, 32, 1e-05, True, False, False, 4, 8),
    ('gn', 'apply', (16, 32, 32, 384), 384, 32, 1e-05, True, False, False, 4, 4),
    ('gn', 'apply', (16, 32, 32, 512), 0, 32, 1e-05, False, False, False, 8, 0),
    ('gn', 'apply', (16, 32, 32, 512), 0, 32, 1e-05, True, False, False, 4, 0),
    ('gn', 'apply', (16, 32, 32, 512), 0, 32, 1e-05, True, False, False, 8, 0),
    ('gn', 'apply', (16, 32, 32, 512), 512, 32, 1e-05, True, False, False, 4, 4),
    ('gn', 'apply', (16, 32, 32, 512), 512, 32, 1e-05, True, False, False, 4, 8),
    ('gn', 'apply', (16, 32, 32, 576), 0, 32, 1e-05, True, True, False, 8, 0),
    ('gn', 'apply', (16, 32, 32, 576), 384, 32, 1e-05, True, False, False, 8, 4),
    ('gn', 'apply', (16, 64, 64, 192), 0, 32, 1e-05, True, False, False, 1, 0),
    ('gn', 'apply', (16, 64, 64, 192), 0, 32, 1e-05, True, True, False, 1, 0),
    ('gn', 'apply', (16, 64, 64, 192), 192, 32, 1e-05, True, False, False, 1, 1),
    ('gn', 'apply', (16, 64, 64, 256), 0, 32, 1e-05, True, False, False, 1, 0),
    ('gn', 'apply', (16, 64, 64, 384), 0, 32, 1e-05, True, True, False, 1, 0),
    ('gn', 'apply', (16, 64, 64, 384), 192, 32, 1e-05, True, False, False, 1, 1),
    ('gn', 'apply', (16, 64, 64, 512), 0, 32, 1e-05, True, False, False, 1, 0),
    ('gn', 'apply', (16, 64, 64, 512), 256, 32, 1e-05, True, False, False, 1, 1),
    ('gn', 'apply', (16, 64, 64, 512), 512, 32, 1e-05, True, False, False, 1, 1),
    ('gn', 'apply', (256, 16, 16, 128), 0, 32, 1e-06, True, False, False, 4, 0),
    ('gn', 'apply', (256, 16, 16, 256), 0, 32, 1e-06, True, False, False, 2, 0),
    ('gn', 'apply', (256, 16, 16, 256), 0, 32, 1e-06, True, False, False, 8, 0),
    ('gn', 'apply', (256, 16, 16, 256), 128, 32, 1e-06, True, False, False, 8, 4),
    ('gn', 'apply', (256, 16, 16, 256), 256, 32, 1e-06, True, False, False, 2, 8),
    ('gn', 'apply', (256, 16, 16, 256), 256, 32, 1e-06, True, False, False, 8, 8),
    ('gn', 'apply', (256, 32, 32, 128), 0, 32, 1e-06, True, False, False, 8, 0),
    ('gn', 'apply', (256, 32, 32, 128), 128, 32, 1e-06, True, False, False, 8, 8),
    ('gn', 'apply', (256, 32, 32, 256), 128, 32, 1e-06, True, False, False, 8, 8),
    ('gn', 'apply', (256, 8, 8, 256), 0, 32, 1e-06, True, False, False, 1, 0),
    ('gn', 'apply', (32, 16, 16, 128), 0, 32, 1e-06, True, False, False, 4, 0),
    ('gn', 'apply', (32, 16, 16, 256), 0, 32, 1e-06, True, False, False, 2, 0),
    ('gn', 'apply', (32, 16, 16, 256), 0, 32, 1e-06, True, False, False, 4, 0),
    ('gn', 'apply', (32, 16, 16, 256), 0, 32, 1e-06, True, False, False, 8, 0),
    ('gn', 'apply', (32, 16, 16, 256), 128, 32, 1e-06, True, False, False, 8, 4),
    ('gn', 'apply', (32, 16, 16, 256), 256, 32, 1e-06, True, False, False, 2, 8),
    ('gn', 'apply', (32, 16, 16, 256), 256, 32, 1e-06, True, False, False, 4, 8),
    ('gn', 'apply', (32, 16, 16, 256), 256, 32, 1e-06, True, False, False, 8, 8),
    ('gn', 'apply', (32, 16, 16, 384), 0, 32, 1e-05, True, False, False, 2, 0),
    ('gn', 'apply', (32, 16, 16, 384), 0, 32, 1e-05, True, True, False, 2, 0),
    ('gn', 'apply', (32, 16, 16, 576), 0, 32, 1e-05, False, False, False, 2, 0),
    ('gn', 'apply', (32, 16, 16, 576), 0, 32, 1e-05, True, False, False, 1, 0),
    ('gn', 'apply', (32, 16, 16, 576), 0, 32, 1e-05, True, True, False, 2, 0),
    ('gn', 'apply', (32, 16, 16, 576), 384, 32, 1e-05, True, False, False, 1, 2),
    ('gn', 'apply', (32, 16, 16, 576), 576, 32, 1e-05, True, False, False, 1, 1),
    ('gn', 'apply', (32, 16, 16, 768), 0, 32, 1e-05, True, True, False, 2, 0),
    ('gn', 'apply', (32, 16, 16, 768), 576, 32, 1e-05, True, False, False, 2, 1),
    ('gn', 'apply', (32, 32, 32, 128), 0, 32, 1e-06, True, False, False, 8, 0),
    ('gn', 'apply', (32, 32, 32, 128), 128, 32, 1e-06, True, False, False, 8, 8),
    ('gn', 'apply', (32, 32, 32, 192), 0, 32, 1e-05, True, False, False, 8, 0),
    ('gn', 'apply', (32, 32, 32, 192), 0, 32, 1e-05, True, True, False, 8, 0),
    ('gn', 'apply', (32, 32, 32, 256), 128, 32, 1e-06, True, False, False, 8, 8),
    ('gn', 'apply', (32, 32, 32, 384), 0, 32, 1e-05, False, False, False, 8, 0),
    ('gn', 'apply', (32, 32, 32, 384), 0, 32, 1e-05, True, False, False, 4, 0),
    ('gn', 'apply', (32, 32, 32, 384), 0, 32, 1e-05, True, True, False, 8, 0),
    ('gn', 'apply', (32, 32, 32, 384), 192, 32, 1e-05, True, False, False, 4, 8),
    ('gn', 'apply', (32, 32, 32, 384), 384, 32, 1e-05, True, False, False, 4, 4),
    ('gn', 'apply', (32, 32, 32, 576), 0, 32, 1e-05, True, True, False, 8, 0),
    ('gn', 'apply', (32, 32, 32, 576), 384, 32, 1e-05, True, False, False, 8, 4),
    ('gn', 'apply', (32, 64, 64, 192), 0, 32, 1e-05, True, False, False, 1, 0),
    ('gn', 'apply', (32, 64, 64, 192), 0, 32, 1e-05, True, True, False, 1, 0),
    ('gn', 'apply', (32, 64, 64, 192), 192, 32, 1e-05, True, False, False, 1, 1),
    ('gn', 'apply', (32, 64, 64, 384), 0, 32, 1e-05, True, True, False, 1, 0),
    ('gn', 'apply', (32, 64, 64, 384), 192, 32, 1e-05, True, False, False, 1, 1),
    ('gn', 'apply', (32, 8, 8, 256), 0, 32, 1e-06, True, False, False, 1, 0),
    ('gn', 'generic', (100, 8, 8, 576), 0, 32, 1e-05, True, False, False, 0, 0),
    ('gn', 'generic', (100, 8, 8, 576), 0, 32, 1e-05, True, True, False, 0, 0),
    ('gn', 'generic', (100, 8, 8, 768), 0, 32, 1e-05, True, True, False, 0, 0),
    ('gn', 'generic', (100, 8, 8, 768), 576, 32, 1e-05, True, False, False, 0, 0),
    ('gn', 'generic', (14, 8, 8, 576), 0, 32, 1e-05, True, False, False, 0, 0),
    ('gn', 'generic', (14, 8, 8, 576), 0, 32, 1e-05, True, True, False, 0, 0),
    ('gn', 'generic', (14, 8, 8, 768), 0, 32, 1e-05, True, True, False, 0, 0),
    ('gn', 'generic', (14, 8, 8, 768), 576, 32, 1e-05, True, False, False, 0, 0),
    ('gn', 'generic', (16, 16, 16, 576), 0, 32, 1e-05, True, True, False, 0, 0),
    ('gn', 'generic', (16, 16, 16, 576), 0, 32, 1e-05, True, True, True, 0, 0),
    ('gn', 'generic', (16, 8, 8, 576), 0, 32, 1e-05, True, False, False, 0, 0),
    ('gn', 'generic', (16, 8, 8, 576), 0, 32, 1e-05, True, False, True, 0, 0),
    ('gn', 'generic', (16, 8, 8, 576), 0, 32, 1e-05, True, True, False, 0, 0),
    ('gn', 'generic', (16, 8, 8, 576), 0, 32, 1e-05, True, True, True, 0, 0),
    ('gn', 'generic', (16, 8, 8, 768), 0, 32, 1e-05, True, True, False, 0, 0),
    ('gn', 'generic', (16, 8, 8, 768), 0, 32, 1e-05, True, True, True, 0, 0),
    ('gn', 'generic', (16, 8, 8, 768), 576, 32, 1e-05, True, False, False, 0, 0),
    ('gn', 'generic', (16, 8, 8, 768), 576, 32, 1e-05, True, False, True, 0, 0),
    ('gn', 'generic', (32, 8, 8, 576), 0, 32, 1e-05, True, False, True, 0, 0),
    ('gn', 'generic', (32, 8, 8, 576), 0, 32, 1e-05, True, True, True, 0, 0),
    ('gn', 'generic', (32, 8, 8, 768), 0, 32, 1e-05, True, True, True, 0, 0),
    ('gn', 'generic', (32, 8, 8, 768), 576, 32, 1e-05, True, False, True, 0, 0),
    ('gn', 'resident', (100, 8, 8, 768), 0, 32, 1e-05, False, False, False, 0, 0),
    ('gn', 'resident', (100, 8, 8, 768), 0, 32, 1e-05, True, False, False, 0, 0),
    ('gn', 'resident', (100, 8, 8, 768), 768, 32, 1e-05, True, False, False, 0, 0),
    ('gn', 'resident', (128, 16, 16, 128), 0, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (128, 16, 16, 256), 0, 32, 1e-06, False, False, False, 0, 0),
    ('gn', 'resident', (128, 16, 16, 256), 0, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (128, 16, 16, 256), 128, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (128, 16, 16, 256), 256, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (128, 32, 32, 128), 0, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (128, 32, 32, 128), 128, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (128, 32, 32, 256), 128, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (128, 4, 4, 256), 0, 32, 1e-06, False, False, False, 0, 0),
    ('gn', 'resident', (128, 4, 4, 256), 0, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (128, 4, 4, 256), 256, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (128, 8, 8, 256), 0, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (128, 8, 8, 256), 256, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (14, 8, 8, 768), 0, 32, 1e-05, False, False, False, 0, 0),
    ('gn', 'resident', (14, 8, 8, 768), 0, 32, 1e-05, True, False, False, 0, 0),
    ('gn', 'resident', (14, 8, 8, 768), 768, 32, 1e-05, True, False, False, 0, 0),
    ('gn', 'resident', (16, 8, 8, 1024), 0, 32, 1e-05, False, False, False, 0, 0),
    ('gn', 'resident', (16, 8, 8, 1024), 0, 32, 1e-05, True, False, False, 0, 0),
    ('gn', 'resident', (16, 8, 8, 1024), 1024, 32, 1e-05, True, False, False, 0, 0),
    ('gn', 'resident', (16, 8, 8, 768), 0, 32, 1e-05, False, False, False, 0, 0),
    ('gn', 'resident', (16, 8, 8, 768), 0, 32, 1e-05, True, False, False, 0, 0),
    ('gn', 'resident', (16, 8, 8, 768), 768, 32, 1e-05, True, False, False, 0, 0),
    ('gn', 'resident', (256, 16, 16, 128), 0, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (256, 16, 16, 256), 0, 32, 1e-06, False, False, False, 0, 0),
    ('gn', 'resident', (256, 16, 16, 256), 0, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (256, 16, 16, 256), 128, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (256, 16, 16, 256), 256, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (256, 32, 32, 128), 0, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (256, 32, 32, 128), 128, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (256, 32, 32, 256), 128, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (256, 4, 4, 256), 0, 32, 1e-06, False, False, False, 0, 0),
    ('gn', 'resident', (256, 4, 4, 256), 0, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (256, 4, 4, 256), 256, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (256, 8, 8, 256), 0, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (256, 8, 8, 256), 256, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (32, 16, 16, 128), 0, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (32, 16, 16, 256), 0, 32, 1e-06, False, False, False, 0, 0),
    ('gn', 'resident', (32, 16, 16, 256), 0, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (32, 16, 16, 256), 128, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (32, 16, 16, 256), 256, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (32, 32, 32, 128), 0, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (32, 32, 32, 128), 128, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (32, 32, 32, 256), 128, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (32, 4, 4, 256), 0, 32, 1e-06, False, False, False, 0, 0),
    ('gn', 'resident', (32, 4, 4, 256), 0, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (32, 4, 4, 256), 256, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (32, 8, 8, 256), 0, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (32, 8, 8, 256), 256, 32, 1e-06, True, False, False, 0, 0),
    ('gn', 'resident', (32, 8, 8, 768), 0, 32, 1e-05, False, False, False, 0, 0),
    ('gn', 'resident', (32, 8, 8, 768), 0, 32, 1e-05, True, False, False, 0, 0),
    ('gn', 'resident', (32, 8, 8, 768), 768, 32, 1e-05, True, False, False, 0, 0),
    ('gn_bs2gen', 16, 1024, 192, 0, 32, 8, 0),
    ('gn_bs2gen', 16, 1024, 384, 0, 32, 4, 0),
    ('gn_bs2gen', 16, 1024, 384, 0, 32, 8, 0),
    ('gn_bs2gen', 16, 1024, 384, 192, 32, 4, 8),
    ('gn_bs2gen', 16, 1024, 384, 384, 32, 4, 4),
    ('gn_bs2gen', 16, 1024, 576, 0, 32, 8, 0),
    ('gn_bs2gen', 16, 1024, 576, 384, 32, 8, 4),
    ('gn_bs2gen', 16, 256, 384, 0, 32, 2, 0),
    ('gn_bs2gen', 16, 256, 384, 0, 32, 4, 0),
    ('gn_bs2gen', 16, 256, 576, 0, 32, 1, 0),
    ('gn_bs2gen', 16, 256, 576, 0, 32, 2, 0),
    ('gn_bs2gen', 16, 256, 576, 384, 32, 1, 2),
    ('gn_bs2gen', 16, 256, 576, 384, 32, 1, 4),
    ('gn_bs2gen', 16, 256, 576, 576, 32, 1, 1),
    ('gn_bs2gen', 16, 256, 768, 0, 32, 2, 0),
    ('gn_bs2gen', 16, 256, 768, 576, 32, 2, 1),
    ('gn_bs2gen', 16, 4096, 192, 0, 32, 1, 0),
    ('gn_bs2gen', 16, 4096, 192, 192, 32, 1, 1),
    ('gn_bs2gen', 16, 4096, 384, 0, 32, 1, 0),
    ('gn_bs2gen', 16, 4096, 384, 192, 32, 1, 1),
    ('gn_bs2gen', 32, 1024, 192, 0, 32, 8, 0),
    ('gn_bs2gen', 32, 1024, 384, 0, 32, 4, 0),
    ('gn_bs2gen', 32, 1024, 384, 0, 32, 8, 0),
    ('gn_bs2gen', 32, 1024, 384, 192, 32, 4, 8),
    ('gn_bs2gen', 32, 1024, 384, 384, 32, 4, 4),
    ('gn_bs2gen', 32, 1024, 576, 0, 32, 8, 0),
    ('gn_bs2gen', 32, 1024, 576, 384, 32, 8, 4),
    ('gn_bs2gen', 32, 256, 384, 0, 32, 2, 0),
    ('gn_bs2gen', 32, 256, 576, 0, 32, 1, 0),
    ('gn_bs2gen', 32, 256, 576, 0, 32, 2, 0),
    ('gn_bs2gen', 32, 256, 576, 384, 32, 1, 2),
    ('gn_bs2gen', 32, 256, 576, 576, 32, 1, 1),
    ('gn_bs2gen', 32, 256, 768, 0, 32, 2, 0),
    ('gn_bs2gen', 32, 256, 768, 576, 32, 2, 1),
    ('gn_bs2gen', 32, 4096, 192, 0, 32, 1, 0),
    ('gn_bs2gen', 32, 4096, 192, 192, 32, 1, 1),
    ('gn_bs2gen', 32, 4096, 384, 0, 32, 1, 0),
    ('gn_bs2gen', 32, 4096, 384, 192, 32, 1, 1),
    ('gn_shortcut', (128, 16, 16, 128), 0, 256, 32, 1e-06, True, True, 4, 0),
    ('gn_shortcut', (128, 16, 16, 256), 128, 256, 32, 1e-06, True, True, 8, 4),
    ('gn_shortcut', (128, 16, 16, 256), 256, 256, 32, 1e-06, True, True, 2, 8),
    ('gn_shortcut', (128, 16, 16, 256), 256, 256, 32, 1e-06, True, True, 8, 8),
    ('gn_shortcut', (128, 32, 32, 128), 128, 128, 32, 1e-06, True, True, 8, 8),
    ('gn_shortcut', (128, 32, 32, 256), 128, 128, 32, 1e-06, True, True, 8, 8),
    ('gn_shortcut', (256, 16, 16, 128), 0, 256, 32, 1e-06, True, True, 4, 0),
    ('gn_shortcut', (256, 16, 16, 256), 128, 256, 32, 1e-06, True, True, 8, 4),
    ('gn_shortcut', (256, 16, 16, 256), 256, 256, 32, 1e-06, True, True, 2, 8),
    ('gn_shortcut', (256, 16, 16, 256), 256, 256, 32, 1e-06, True, True, 8, 8),
    ('gn_shortcut', (256, 32, 32, 128), 128, 128, 32, 1e-06, True, True, 8, 8),
    ('gn_shortcut', (256, 32, 32, 256), 128, 128, 32, 1e-06, True, True, 8, 8),
    ('gn_shortcut', (32, 32, 32, 128), 128, 128, 32, 1e-06, True, True, 8, 8),
    ('gn_shortcut', (32, 32, 32, 256), 128, 128, 32, 1e-06, True, True, 8, 8),
    ('karras_stage', 0, False, (100, 3, 64, 64), ('x2', 'd', 'x_in', 't')),
    ('karras_stage', 1, False, (100, 3, 64, 64), ('x2', 'd', 'model_out', 'x_in', 't')),
    ('karras_stage', 2, False, (100, 3, 64, 64), ('x2', 'd', 'model_out', 'x_in', 't')),
    ('karras_stage', 4, True, (100, 3, 64, 64), ('x2', 'd', 'model_out', 'out')),
    ('linear', 10, 128, 512, 0, 3, True, 'small', 1),
    ('linear', 10, 512, 4992, 0, 0, True, 'small', 1),
    ('linear', 10, 512, 512, 0, 3, True, 'small', 1),
    ('linear', 100, 192, 768, 0, 3, True, 'small', 1),
    ('linear', 100, 768, 35712, 3, 0, True, 'small', 1),
    ('linear', 100, 768, 768, 0, 0, True, 'small', 1),
    ('linear', 128, 128, 512, 0, 3, True, 'small', 1),
    ('linear', 128, 512, 4992, 0, 0, True, 'small', 1),
    ('linear', 128, 512, 512, 0, 3, True, 'small', 1),
    ('linear', 14, 192, 768, 0, 3, True, 'small', 1),
    ('linear', 14, 768, 35712, 3, 0, True, 'small', 1),
    ('linear', 14, 768, 768, 0, 0, True, 'small', 1),
    ('linear', 16, 1024, 1024, 0, 0, True, 'small', 1),
    ('linear', 16, 1024, 25856, 3, 0, True, 'small', 1),
    ('linear', 16, 192, 768, 0, 3, True, 'small', 1),
    ('linear', 16, 256, 1024, 0, 3, True, 'small', 1),
    ('linear', 16, 768, 35712, 3, 0, True, 'small', 1),
    ('linear', 16, 768, 768, 0, 0, True, 'small', 1),
    ('linear', 256, 128, 512, 0, 3, True, 'small', 1),
    ('linear', 256, 512, 4992, 0, 0, True, 'small', 1),
    ('linear', 256, 512, 512, 0, 3, True, 'small', 1),
    ('linear', 32, 128, 512, 0, 3, True, 'small', 1),
    ('linear', 32, 192, 768, 0, 3, True, 'small', 1),
    ('linear', 32, 512, 4992, 0, 0, True, 'small', 1),
    ('linear', 32, 512, 512, 0, 3, True, 'small', 1),
    ('linear', 32, 768, 35712, 3, 0, True, 'small', 1),
    ('linear', 32, 768, 768, 0, 0, True, 'small', 1),
    ('linear', 4, 128, 512, 0, 3, True, 'small', 1),
    ('linear', 4, 512, 4992, 0, 0, True, 'small', 1),
    ('linear', 4, 512, 512, 0, 3, True, 'small', 1),
    ('pool_act', (100, 16, 16, 576), True, 0),
    ('pool_act', (100, 32, 32, 384), True, 0),
    ('pool_act', (100, 64, 64, 192), True, 0),
    ('pool_act', (128, 16, 16, 256), True, 1),
    ('pool_act', (128, 32, 32, 128), True, 1),
    ('pool_act', (128, 8, 8, 256), True, 1),
    ('pool_act', (14, 16, 16, 576), True, 0),
    ('pool_act', (14, 32, 32, 384), True, 0),
    ('pool_act', (14, 64, 64, 192), True, 0),
    ('pool_act', (16, 128, 128, 256), True, 0),
    ('pool_act', (16, 16, 16, 1024), True, 0),
    ('pool_act', (16, 16, 16, 256), True, 1),
    ('pool_act', (16, 16, 16, 576), True, 0),
    ('pool_act', (16, 256, 256, 256), True, 0),
    ('pool_act', (16, 32, 32, 256), True, 1),
    ('pool_act', (16, 32, 32, 384), True, 0),
    ('pool_act', (16, 32, 32, 512), True, 0),
    ('pool_act', (16, 64, 64, 128), True, 1),
    ('pool_act', (16, 64, 64, 192), True, 0),
    ('pool_act', (16, 64, 64, 512), True, 0),
    ('pool_act', (256, 16, 16, 256), True, 1),
    ('pool_act', (256, 32, 32, 128), True, 1),
    ('pool_act', (256, 8, 8, 256), True, 1),
    ('pool_act', (32, 16, 16, 256), True, 1),
    ('pool_act', (32, 16, 16, 576), True, 0),
    ('pool_act', (32, 32, 32, 128), True, 1),
    ('pool_act', (32, 32, 32, 256), True, 1),
    ('pool_act', (32, 32, 32, 384), True, 0),
    ('pool_act', (32, 64, 64, 128), True, 1),
    ('pool_act', (32, 64, 64, 192), True, 0),
    ('pool_act', (32, 8, 8, 256), True, 1),
    ('pool_act', (512, 16, 16, 256), True, 1),
    ('pool_act', (512, 32, 32, 128), True, 1),
    ('pool_act', (512, 8, 8, 256), True, 1),
    ('pool_act', (64, 16, 16, 256), True, 1),
    ('pool_act', (64, 32, 32, 128), True, 1),
    ('pool_act', (64, 8, 8, 256), True, 1),
    ('td_gather_cost', 128, 3072, ('next_rows',)),
    ('td_gather_cost', 256, 3072, ('next_rows',)),
    ('td_gather_cost', 32, 3072, ('next_rows',)),
    ('td_loss', 128, True),
    ('td_loss', 256, True),
    ('td_loss', 32, True),
    ('timestep_embedding', 10, 128, 0, 10000.0),
    ('timestep_embedding', 100, 192, 1, 10000.0),
    ('timestep_embedding', 128, 128, 0, 10000.0),
    ('timestep_embedding', 14, 192, 1, 10000.0),
    ('timestep_embedding', 16, 192, 1, 10000.0),
    ('timestep_embedding', 16, 256, 1, 10000.0),
    ('timestep_embedding', 256, 128, 0, 10000.0),
    ('timestep_embedding', 32, 128, 0, 10000.0),
    ('timestep_embedding', 32, 192, 1, 10000.0),
    ('timestep_embedding', 4, 128, 0, 10000.0),
    ('upsample2x', (100, 16, 16, 576)),
    ('upsample2x', (100, 32, 32, 384)),
    ('upsample2x', (100, 8, 8, 768)),
    ('upsample2x', (14, 16, 16, 576)),
    ('upsample2x', (14, 32, 32, 384)),
    ('upsample2x', (14, 8, 8, 768)),
    ('upsample2x', (16, 128, 128, 256)),
    ('upsample2x', (16, 16, 16, 1024)),
    ('upsample2x', (16, 16, 16, 576)),
    ('upsample2x', (16, 32, 32, 384)),
    ('upsample2x', (16, 32, 32, 512)),
    ('upsample2x', (16, 64, 64, 512)),
    ('upsample2x', (16, 8, 8, 1024)),
    ('upsample2x', (16, 8, 8, 768)),
    ('upsample2x', (32, 16, 16, 576)),
    ('upsample2x', (32, 32, 32, 384)),
    ('upsample2x', (32, 8, 8, 768)),
    ('value_head', (128, 4, 4, 256), True),
    ('value_head', (16, 8, 8, 256), True),
    ('value_head', (256, 4, 4, 256), True),
    ('value_head', (32, 4, 4, 256), True),
    ('value_head', (32, 8, 8, 256), True),
    ('value_head', (512, 4, 4, 256), True),
    ('value_head', (64, 4, 4, 256), True),
    ('var_gather_sched', 128, 10),
    ('var_gather_sched', 128, 4),
    ('var_gather_sched', 256, 10),
    ('var_gather_sched', 32, 10),
    ('var_step', (128, 3, 32, 32), True, True, 0),
    ('var_step', (128, 3, 32, 32), True, True, 1),
    ('var_step', (256, 3, 32, 32), True, True, 0),
    ('var_step', (256, 3, 32, 32), True, True, 1),
    ('var_step', (32, 3, 32, 32), True, True, 0),
    ('var_step', (32, 3, 32, 32), True, True, 1),
]

COND = {
    ('gn', 'apply', (100, 16, 16, 384), 0, 32, 1e-05, True, False, False, 2, 0): 0.824,
    ('gn', 'apply', (100, 16, 16, 384), 0, 32, 1e-05, True, True, False, 2, 0): 1.098,
    ('gn', 'apply', (100, 16, 16, 576), 0, 32, 1e-05, False, False, False, 2, 0): 0.795,
    ('gn', 'apply', (100, 16, 16, 576), 0, 32, 1e-05, True, False, False, 1, 0): 0.847,
    ('gn', 'apply', (100, 16, 16, 576), 0, 32, 1e-05, True, True, False, 2, 0): 0.837,
    ('gn', 'apply', (100, 16, 16, 576), 384, 32, 1e-05, True, False, False, 1, 2): 0.486,
    ('gn', 'apply', (100, 16, 16, 576), 576, 32, 1e-05, True, False, False, 1, 1): 0.607,
    ('gn', 'apply', (100, 16, 16, 768), 0, 32, 1e-05, True, True, False, 2, 0): 0.638,
    ('gn', 'apply', (100, 16, 16, 768), 576, 32, 1e-05, True, False, False, 2, 1): 0.417,
    ('gn', 'apply', (100, 32, 32, 192), 0, 32, 1e-05, True, False, False, 8, 0): 1.424,
    ('gn', 'apply', (100, 32, 32, 192), 0, 32, 1e-05, True, True, False, 8, 0): 1.326,
    ('gn', 'apply', (100, 32, 32, 384), 0, 32, 1e-05, False, False, False, 8, 0): 0.976,
    ('gn', 'apply', (100, 32, 32, 384), 0, 32, 1e-05, True, False, False, 4, 0): 0.877,
    ('gn', 'apply', (100, 32, 32, 384), 0, 32, 1e-05, True, True, False, 8, 0): 0.959,
    ('gn', 'apply', (100, 32, 32, 384), 192, 32, 1e-05, True, False, False, 4, 8): 0.804,
    ('gn', 'apply', (100, 32, 32, 384), 384, 32, 1e-05, True, False, False, 4, 4): 0.596,
    ('gn', 'apply', (100, 32, 32, 576), 0, 32, 1e-05, True, True, False, 8, 0): 0.872,
    ('gn', 'apply', (100, 32, 32, 576), 384, 32, 1e-05, True, False, False, 8, 4): 0.503,
    ('gn', 'apply', (100, 64, 64, 192), 0, 32, 1e-05, True, False, False, 1, 0): 0.826,
    ('gn', 'apply', (100, 64, 64, 192), 0, 32, 1e-05, True, True, False, 1, 0): 1.053,
    ('gn', 'apply', (100, 64, 64, 192), 192, 32, 1e-05, True, False, False, 1, 1): 0.874,
    ('gn', 'apply', (100, 64, 64, 384), 0, 32, 1e-05, True, True, False, 1, 0): 0.859,
    ('gn', 'apply', (100, 64, 64, 384), 192, 32, 1e-05, True, False, False, 1, 1): 0.71,
    ('gn', 'apply', (128, 16, 16, 128), 0, 32, 1e-06, True, False, False, 4, 0): 0.373,
    ('gn', 'apply', (128, 16, 16, 256), 0, 32, 1e-06, True, False, False, 2, 0): 0.581,
    ('gn', 'apply', (128, 16, 16, 256), 0, 32, 1e-06, True, False, False, 8, 0): 0.443,
    ('gn', 'apply', (128, 16, 16, 256), 128, 32, 1e-06, True, False, False, 8, 4): 0.368,
    ('gn', 'apply', (128, 16, 16, 256), 256, 32, 1e-06, True, False, False, 2, 8): 0.373,
    ('gn', 'apply', (128, 16, 16, 256), 256, 32, 1e-06, True, False, False, 8, 8): 0.43,
    ('gn', 'apply', (128, 32, 32, 128), 0, 32, 1e-06, True, False, False, 8, 0): 0.839,
    ('gn', 'apply', (128, 32, 32, 128), 128, 32, 1e-06, True, False, False, 8, 8): 0.499,
    ('gn', 'apply', (128, 32, 32, 256), 128, 32, 1e-06, True, False, False, 8, 8): 0.357,
    ('gn', 'apply', (128, 8, 8, 256), 0, 32, 1e-06, True, False, False, 1, 0): 0.626,
    ('gn', 'apply', (14, 16, 16, 384), 0, 32, 1e-05, True, False, False, 2, 0): 0.727,
    ('gn', 'apply', (14, 16, 16, 384), 0, 32, 1e-05, True, True, False, 2, 0): 1.077,
    ('gn', 'apply', (14, 16, 16, 576), 0, 32, 1e-05, False, False, False, 2, 0): 0.702,
    ('gn', 'apply', (14, 16, 16, 576), 0, 32, 1e-05, True, False, False, 1, 0): 0.707,
    ('gn', 'apply', (14, 16, 16, 576), 0, 32, 1e-05, True, True, False, 2, 0): 0.817,
    ('gn', 'apply', (14, 16, 16, 576), 384, 32, 1e-05, True, False, False, 1, 2): 0.446,
    ('gn', 'apply', (14, 16, 16, 576), 576, 32, 1e-05, True, False, False, 1, 1): 0.495,
    ('gn', 'apply', (14, 16, 16, 768), 0, 32, 1e-05, True, True, False, 2, 0): 0.512,
    ('gn', 'apply', (14, 16, 16, 768), 576, 32, 1e-05, True, False, False, 2, 1): 0.331,
    ('gn', 'apply', (14, 32, 32, 192), 0, 32, 1e-05, True, False, False, 8, 0): 1.113,
    ('gn', 'apply', (14, 32, 32, 192), 0, 32, 1e-05, True, True, False, 8, 0): 1.265,
    ('gn', 'apply', (14, 32, 32, 384), 0, 32, 1e-05, False, False, False, 8, 0): 0.864,
    ('gn', 'apply', (14, 32, 32, 384), 0, 32, 1e-05, True, False, False, 4, 0): 0.716,
    ('gn', 'apply', (14, 32, 32, 384), 0, 32, 1e-05, True, True, False, 8, 0): 0.83,
    ('gn', 'apply', (14, 32, 32, 384), 192, 32, 1e-05, True, False, False, 4, 8): 0.696,
    ('gn', 'apply', (14, 32, 32, 384), 384, 32, 1e-05, True, False, False, 4, 4): 0.53,
    ('gn', 'apply', (14, 32, 32, 576), 0, 32, 1e-05, True, True, False, 8, 0): 0.692,
    ('gn', 'apply', (14, 32, 32, 576), 384, 32, 1e-05, True, False, False, 8, 4): 0.381,
    ('gn', 'apply', (14, 64, 64, 192), 0, 32, 1e-05, True, False, False, 1, 0): 0.766,
    ('gn', 'apply', (14, 64, 64, 192), 0, 32, 1e-05, True, True, False, 1, 0): 0.91,
    ('gn', 'apply', (14, 64, 64, 192), 192, 32, 1e-05, True, False, False, 1, 1): 0.715,
    ('gn', 'apply', (14, 64, 64, 384), 0, 32, 1e-05, True, True, False, 1, 0): 0.744,
    ('gn', 'apply', (14, 64, 64, 384), 192, 32, 1e-05, True, False, False, 1, 1): 0.503,
    ('gn', 'apply', (16, 128, 128, 256), 0, 32, 1e-05, True, False, False, 4, 0): 1.083,
    ('gn', 'apply', (16, 128, 128, 256), 256, 32, 1e-05, True, False, False, 4, 4): 0.447,
    ('gn', 'apply', (16, 128, 128, 512), 0, 32, 1e-05, True, False, False, 4, 0): 0.492,
    ('gn', 'apply', (16, 128, 128, 512), 256, 32, 1e-05, True, False, False, 4, 4): 0.384,
    ('gn', 'apply', (16, 16, 16, 1024), 0, 32, 1e-05, False, False, False, 2, 0): 0.524,
    ('gn', 'apply', (16, 16, 16, 1024), 0, 32, 1e-05, True, False, False, 1, 0): 0.474,
    ('gn', 'apply', (16, 16, 16, 1024), 0, 32, 1e-05, True, False, False, 2, 0): 0.541,
    ('gn', 'apply', (16, 16, 16, 1024), 1024, 32, 1e-05, True, False, False, 1, 1): 0.414,
    ('gn', 'apply', (16, 16, 16, 1024), 1024, 32, 1e-05, True, False, False, 2, 1): 0.284,
    ('gn', 'apply', (16, 16, 16, 1024), 512, 32, 1e-05, True, False, False, 1, 2): 0.425,
    ('gn', 'apply', (16, 16, 16, 384), 0, 32, 1e-05, True, False, False, 2, 0): 0.908,
    ('gn', 'apply', (16, 16, 16, 384), 0, 32, 1e-05, True, False, False, 4, 0): 0.896,
    ('gn', 'apply', (16, 16, 16, 384), 0, 32, 1e-05, True, True, False, 2, 0): 0.665,
    ('gn', 'apply', (16, 16, 16, 384), 0, 32, 1e-05, True, True, False, 4, 0): 1.28,
    ('gn', 'apply', (16, 16, 16, 512), 0, 32, 1e-05, True, False, False, 2, 0): 0.94,
    ('gn', 'apply', (16, 16, 16, 576), 0, 32, 1e-05, False, False, False, 1, 0): 0.809,
    ('gn', 'apply', (16, 16, 16, 576), 0, 32, 1e-05, False, False, False, 2, 0): 0.69,
    ('gn', 'apply', (16, 16, 16, 576), 0, 32, 1e-05, True, False, False, 1, 0): 0.792,
    ('gn', 'apply', (16, 16, 16, 576), 0, 32, 1e-05, True, True, False, 2, 0): 0.65,
    ('gn', 'apply', (16, 16, 16, 576), 384, 32, 1e-05, True, False, False, 1, 2): 0.438,
    ('gn', 'apply', (16, 16, 16, 576), 384, 32, 1e-05, True, False, False, 1, 4): 0.468,
    ('gn', 'apply', (16, 16, 16, 576), 576, 32, 1e-05, True, False, False, 1, 1): 0.503,
    ('gn', 'apply', (16, 16, 16, 768), 0, 32, 1e-05, True, True, False, 2, 0): 0.583,
    ('gn', 'apply', (16, 16, 16, 768), 576, 32, 1e-05, True, False, False, 2, 1): 0.346,
    ('gn', 'apply', (16, 256, 256, 256), 0, 32, 1e-05, True, False, False, 1, 0): 0.602,
    ('gn', 'apply', (16, 256, 256, 256), 0, 32, 1e-05, True, False, False, 8, 0): 0.289,
    ('gn', 'apply', (16, 256, 256, 256), 256, 32, 1e-05, True, False, False, 1, 1): 0.379,
    ('gn', 'apply', (16, 256, 256, 256), 256, 32, 1e-05, True, False, False, 1, 8): 0.295,
    ('gn', 'apply', (16, 32, 32, 1024), 0, 32, 1e-05, True, False, False, 8, 0): 0.364,
    ('gn', 'apply', (16, 32, 32, 1024), 512, 32, 1e-05, True, False, False, 8, 4): 0.328,
    ('gn', 'apply', (16, 32, 32, 192), 0, 32, 1e-05, True, False, False, 8, 0): 1.316,
    ('gn', 'apply', (16, 32, 32, 192), 0, 32, 1e-05, True, True, False, 8, 0): 1.159,
    ('gn', 'apply', (16, 32, 32, 384), 0, 32, 1e-05, False, False, False, 8, 0): 0.902,
    ('gn', 'apply', (16, 32, 32, 384), 0, 32, 1e-05, True, False, False, 4, 0): 0.946,
    ('gn', 'apply', (16, 32, 32, 384), 0, 32, 1e-05, True, True, False, 8, 0): 0.933,
    ('gn', 'apply', (16, 32, 32, 384), 192, 32, 1e-05, True, False, False, 4, 8): 0.679,
    ('gn', 'apply', (16, 32, 32, 384), 384, 32, 1e-05, True, False, False, 4, 4): 0.563,
    ('gn', 'apply', (16, 32, 32, 512), 0, 32, 1e-05, False, False, False, 8, 0): 0.817,
    ('gn', 'apply', (16, 32, 32, 512), 0, 32, 1e-05, True, False, False, 4, 0): 0.855,
    ('gn', 'apply', (16, 32, 32, 512), 0, 32, 1e-05, True, False, False, 8, 0): 0.822,
    ('gn', 'apply', (16, 32, 32, 512), 512, 32, 1e-05, True, False, False, 4, 4): 0.473,
    ('gn', 'apply', (16, 32, 32, 512), 512, 32, 1e-05, True, False, False, 4, 8): 0.491,
    ('gn', 'apply', (16, 32, 32, 576), 0, 32, 1e-05, True, True, False, 8, 0): 0.688,
    ('gn', 'apply', (16, 32, 32, 576), 384, 32, 1e-05, True, False, False, 8, 4): 0.418,
    ('gn', 'apply', (16, 64, 64, 192), 0, 32, 1e-05, True, False, False, 1, 0): 0.791,
    ('gn', 'apply', (16, 64, 64, 192), 0, 32, 1e-05, True, True, False, 1, 0): 0.984,
    ('gn', 'apply', (16, 64, 64, 192), 192, 32, 1e-05, True, False, False, 1, 1): 0.704,
    ('gn', 'apply', (16, 64, 64, 256), 0, 32, 1e-05, True, False, False, 1, 0): 0.939,
    ('gn', 'apply', (16, 64, 64, 384), 0, 32, 1e-05, True, True, False, 1, 0): 0.677,
    ('gn', 'apply', (16, 64, 64, 384), 192, 32, 1e-05, True, False, False, 1, 1): 0.601,
    ('gn', 'apply', (16, 64, 64, 512), 0, 32, 1e-05, True, False, False, 1, 0): 0.646,
    ('gn', 'apply', (16, 64, 64, 512), 256, 32, 1e-05, True, False, False, 1, 1): 0.434,
    ('gn', 'apply', (16, 64, 64, 512), 512, 32, 1e-05, True, False, False, 1, 1): 0.374,
    ('gn', 'apply', (256, 16, 16, 128), 0, 32, 1e-06, True, False, False, 4, 0): 0.373,
    ('gn', 'apply', (256, 16, 16, 256), 0, 32, 1e-06, True, False, False, 2, 0): 0.525,
    ('gn', 'apply', (256, 16, 16, 256), 0, 32, 1e-06, True, False, False, 8, 0): 0.443,
    ('gn', 'apply', (256, 16, 16, 256), 128, 32, 1e-06, True, False, False, 8, 4): 0.356,
    ('gn', 'apply', (256, 16, 16, 256), 256, 32, 1e-06, True, False, False, 2, 8): 0.373,
    ('gn', 'apply', (256, 16, 16, 256), 256, 32, 1e-06, True, False, False, 8, 8): 0.376,
    ('gn', 'apply', (256, 32, 32, 128), 0, 32, 1e-06, True, False, False, 8, 0): 0.84,
    ('gn', 'apply', (256, 32, 32, 128), 128, 32, 1e-06, True, False, False, 8, 8): 0.499,
    ('gn', 'apply', (256, 32, 32, 256), 128, 32, 1e-06, True, False, False, 8, 8): 0.366,
    ('gn', 'apply', (256, 8, 8, 256), 0, 32, 1e-06, True, False, False, 1, 0): 0.626,
    ('gn', 'apply', (32, 16, 16, 128), 0, 32, 1e-06, True, False, False, 4, 0): 0.349,
    ('gn', 'apply', (32, 16, 16, 256), 0, 32, 1e-06, True, False, False, 2, 0): 0.497,
    ('gn', 'apply', (32, 16, 16, 256), 0, 32, 1e-06, True, False, False, 4, 0): 0.497,
    ('gn', 'apply', (32, 16, 16, 256), 0, 32, 1e-06, True, False, False, 8, 0): 0.422,
    ('gn', 'apply', (32, 16, 16, 256), 128, 32, 1e-06, True, False, False, 8, 4): 0.356,
    ('gn', 'apply', (32, 16, 16, 256), 256, 32, 1e-06, True, False, False, 2, 8): 0.335,
    ('gn', 'apply', (32, 16, 16, 256), 256, 32, 1e-06, True, False, False, 4, 8): 0.335,
    ('gn', 'apply', (32, 16, 16, 256), 256, 32, 1e-06, True, False, False, 8, 8): 0.359,
    ('gn', 'apply', (32, 16, 16, 384), 0, 32, 1e-05, True, False, False, 2, 0): 0.908,
    ('gn', 'apply', (32, 16, 16, 384), 0, 32, 1e-05, True, True, False, 2, 0): 0.665,
    ('gn', 'apply', (32, 16, 16, 576), 0, 32, 1e-05, False, False, False, 2, 0): 0.809,
    ('gn', 'apply', (32, 16, 16, 576), 0, 32, 1e-05, True, False, False, 1, 0): 0.829,
    ('gn', 'apply', (32, 16, 16, 576), 0, 32, 1e-05, True, True, False, 2, 0): 0.693,
    ('gn', 'apply', (32, 16, 16, 576), 384, 32, 1e-05, True, False, False, 1, 2): 0.48,
    ('gn', 'apply', (32, 16, 16, 576), 576, 32, 1e-05, True, False, False, 1, 1): 0.442,
    ('gn', 'apply', (32, 16, 16, 768), 0, 32, 1e-05, True, True, False, 2, 0): 0.591,
    ('gn', 'apply', (32, 16, 16, 768), 576, 32, 1e-05, True, False, False, 2, 1): 0.399,
    ('gn', 'apply', (32, 32, 32, 128), 0, 32, 1e-06, True, False, False, 8, 0): 0.84,
    ('gn', 'apply', (32, 32, 32, 128), 128, 32, 1e-06, True, False, False, 8, 8): 0.499,
    ('gn', 'apply', (32, 32, 32, 192), 0, 32, 1e-05, True, False, False, 8, 0): 1.115,
    ('gn', 'apply', (32, 32, 32, 192), 0, 32, 1e-05, True, True, False, 8, 0): 0.871,
    ('gn', 'apply', (32, 32, 32, 256), 128, 32, 1e-06, True, False, False, 8, 8): 0.343,
    ('gn', 'apply', (32, 32, 32, 384), 0, 32, 1e-05, False, False, False, 8, 0): 0.774,
    ('gn', 'apply', (32, 32, 32, 384), 0, 32, 1e-05, True, False, False, 4, 0): 0.709,
    ('gn', 'apply', (32, 32, 32, 384), 0, 32, 1e-05, True, True, False, 8, 0): 0.876,
    ('gn', 'apply', (32, 32, 32, 384), 192, 32, 1e-05, True, False, False, 4, 8): 0.463,
    ('gn', 'apply', (32, 32, 32, 384), 384, 32, 1e-05, True, False, False, 4, 4): 0.505,
    ('gn', 'apply', (32, 32, 32, 576), 0, 32, 1e-05, True, True, False, 8, 0): 0.589,
    ('gn', 'apply', (32, 32, 32, 576), 384, 32, 1e-05, True, False, False, 8, 4): 0.507,
    ('gn', 'apply', (32, 64, 64, 192), 0, 32, 1e-05, True, False, False, 1, 0): 0.724,
    ('gn', 'apply', (32, 64, 64, 192), 0, 32, 1e-05, True, True, False, 1, 0): 0.75,
    ('gn', 'apply', (32, 64, 64, 192), 192, 32, 1e-05, True, False, False, 1, 1): 0.595,
    ('gn', 'apply', (32, 64, 64, 384), 0, 32, 1e-05, True, True, False, 1, 0): 0.562,
    ('gn', 'apply', (32, 64, 64, 384), 192, 32, 1e-05, True, False, False, 1, 1): 0.484,
    ('gn', 'apply', (32, 8, 8, 256), 0, 32, 1e-06, True, False, False, 1, 0): 0.626,
    ('gn', 'generic', (100, 8, 8, 576), 0, 32, 1e-05, True, False, False, 0, 0): 0.87,
    ('gn', 'generic', (100, 8, 8, 576), 0, 32, 1e-05, True, True, False, 0, 0): 0.871,
    ('gn', 'generic', (100, 8, 8, 768), 0, 32, 1e-05, True, True, False, 0, 0): 0.707,
    ('gn', 'generic', (100, 8, 8, 768), 576, 32, 1e-05, True, False, False, 0, 0): 0.569,
    ('gn', 'generic', (14, 8, 8, 576), 0, 32, 1e-05, True, False, False, 0, 0): 0.667,
    ('gn', 'generic', (14, 8, 8, 576), 0, 32, 1e-05, True, True, False, 0, 0): 0.758,
    ('gn', 'generic', (14, 8, 8, 768), 0, 32, 1e-05, True, True, False, 0, 0): 0.615,
    ('gn', 'generic', (14, 8, 8, 768), 576, 32, 1e-05, True, False, False, 0, 0): 0.503,
    ('gn', 'generic', (16, 16, 16, 576), 0, 32, 1e-05, True, True, False, 0, 0): 0.783,
    ('gn', 'generic', (16, 16, 16, 576), 0, 32, 1e-05, True, True, True, 0, 0): 0.783,
    ('gn', 'generic', (16, 8, 8, 576), 0, 32, 1e-05, True, False, False, 0, 0): 0.76,
    ('gn', 'generic', (16, 8, 8, 576), 0, 32, 1e-05, True, False, True, 0, 0): 0.76,
    ('gn', 'generic', (16, 8, 8, 576), 0, 32, 1e-05, True, True, False, 0, 0): 0.817,
    ('gn', 'generic', (16, 8, 8, 576), 0, 32, 1e-05, True, True, True, 0, 0): 0.817,
    ('gn', 'generic', (16, 8, 8, 768), 0, 32, 1e-05, True, True, False, 0, 0): 0.584,
    ('gn', 'generic', (16, 8, 8, 768), 0, 32, 1e-05, True, True, True, 0, 0): 0.584,
    ('gn', 'generic', (16, 8, 8, 768), 576, 32, 1e-05, True, False, False, 0, 0): 0.438,
    ('gn', 'generic', (16, 8, 8, 768), 576, 32, 1e-05, True, False, True, 0, 0): 0.438,
    ('gn', 'generic', (32, 8, 8, 576), 0, 32, 1e-05, True, False, True, 0, 0): 0.729,
    ('gn', 'generic', (32, 8, 8, 576), 0, 32, 1e-05, True, True, True, 0, 0): 0.705,
    ('gn', 'generic', (32, 8, 8, 768), 0, 32, 1e-05, True, True, True, 0, 0): 0.53,
    ('gn', 'generic', (32, 8, 8, 768), 576, 32, 1e-05, True, False, True, 0, 0): 0.524,
    ('gn', 'resident', (100, 8, 8, 768), 0, 32, 1e-05, False, False, False, 0, 0): 0.776,
    ('gn', 'resident', (100, 8, 8, 768), 0, 32, 1e-05, True, False, False, 0, 0): 0.746,
    ('gn', 'resident', (100, 8, 8, 768), 768, 32, 1e-05, True, False, False, 0, 0): 0.491,
    ('gn', 'resident', (128, 16, 16, 128), 0, 32, 1e-06, True, False, False, 0, 0): 0.372,
    ('gn', 'resident', (128, 16, 16, 256), 0, 32, 1e-06, False, False, False, 0, 0): 0.48,
    ('gn', 'resident', (128, 16, 16, 256), 0, 32, 1e-06, True, False, False, 0, 0): 0.452,
    ('gn', 'resident', (128, 16, 16, 256), 128, 32, 1e-06, True, False, False, 0, 0): 0.322,
    ('gn', 'resident', (128, 16, 16, 256), 256, 32, 1e-06, True, False, False, 0, 0): 0.338,
    ('gn', 'resident', (128, 32, 32, 128), 0, 32, 1e-06, True, False, False, 0, 0): 0.756,
    ('gn', 'resident', (128, 32, 32, 128), 128, 32, 1e-06, True, False, False, 0, 0): 0.463,
    ('gn', 'resident', (128, 32, 32, 256), 128, 32, 1e-06, True, False, False, 0, 0): 0.327,
    ('gn', 'resident', (128, 4, 4, 256), 0, 32, 1e-06, False, False, False, 0, 0): 0.426,
    ('gn', 'resident', (128, 4, 4, 256), 0, 32, 1e-06, True, False, False, 0, 0): 0.695,
    ('gn', 'resident', (128, 4, 4, 256), 256, 32, 1e-06, True, False, False, 0, 0): 0.537,
    ('gn', 'resident', (128, 8, 8, 256), 0, 32, 1e-06, True, False, False, 0, 0): 0.615,
    ('gn', 'resident', (128, 8, 8, 256), 256, 32, 1e-06, True, False, False, 0, 0): 0.43,
    ('gn', 'resident', (14, 8, 8, 768), 0, 32, 1e-05, False, False, False, 0, 0): 0.652,
    ('gn', 'resident', (14, 8, 8, 768), 0, 32, 1e-05, True, False, False, 0, 0): 0.634,
    ('gn', 'resident', (14, 8, 8, 768), 768, 32, 1e-05, True, False, False, 0, 0): 0.461,
    ('gn', 'resident', (16, 8, 8, 1024), 0, 32, 1e-05, False, False, False, 0, 0): 0.527,
    ('gn', 'resident', (16, 8, 8, 1024), 0, 32, 1e-05, True, False, False, 0, 0): 0.506,
    ('gn', 'resident', (16, 8, 8, 1024), 1024, 32, 1e-05, True, False, False, 0, 0): 0.311,
    ('gn', 'resident', (16, 8, 8, 768), 0, 32, 1e-05, False, False, False, 0, 0): 0.677,
    ('gn', 'resident', (16, 8, 8, 768), 0, 32, 1e-05, True, False, False, 0, 0): 0.637,
    ('gn', 'resident', (16, 8, 8, 768), 768, 32, 1e-05, True, False, False, 0, 0): 0.441,
    ('gn', 'resident', (256, 16, 16, 128), 0, 32, 1e-06, True, False, False, 0, 0): 0.343,
    ('gn', 'resident', (256, 16, 16, 256), 0, 32, 1e-06, False, False, False, 0, 0): 0.516,
    ('gn', 'resident', (256, 16, 16, 256), 0, 32, 1e-06, True, False, False, 0, 0): 0.474,
    ('gn', 'resident', (256, 16, 16, 256), 128, 32, 1e-06, True, False, False, 0, 0): 0.327,
    ('gn', 'resident', (256, 16, 16, 256), 256, 32, 1e-06, True, False, False, 0, 0): 0.337,
    ('gn', 'resident', (256, 32, 32, 128), 0, 32, 1e-06, True, False, False, 0, 0): 0.793,
    ('gn', 'resident', (256, 32, 32, 128), 128, 32, 1e-06, True, False, False, 0, 0): 0.463,
    ('gn', 'resident', (256, 32, 32, 256), 128, 32, 1e-06, True, False, False, 0, 0): 0.327,
    ('gn', 'resident', (256, 4, 4, 256), 0, 32, 1e-06, False, False, False, 0, 0): 0.495,
    ('gn', 'resident', (256, 4, 4, 256), 0, 32, 1e-06, True, False, False, 0, 0): 0.675,
    ('gn', 'resident', (256, 4, 4, 256), 256, 32, 1e-06, True, False, False, 0, 0): 0.534,
    ('gn', 'resident', (256, 8, 8, 256), 0, 32, 1e-06, True, False, False, 0, 0): 0.613,
    ('gn', 'resident', (256, 8, 8, 256), 256, 32, 1e-06, True, False, False, 0, 0): 0.427,
    ('gn', 'resident', (32, 16, 16, 128), 0, 32, 1e-06, True, False, False, 0, 0): 0.317,
    ('gn', 'resident', (32, 16, 16, 256), 0, 32, 1e-06, False, False, False, 0, 0): 0.479,
    ('gn', 'resident', (32, 16, 16, 256), 0, 32, 1e-06, True, False, False, 0, 0): 0.449,
    ('gn', 'resident', (32, 16, 16, 256), 128, 32, 1e-06, True, False, False, 0, 0): 0.301,
    ('gn', 'resident', (32, 16, 16, 256), 256, 32, 1e-06, True, False, False, 0, 0): 0.32,
    ('gn', 'resident', (32, 32, 32, 128), 0, 32, 1e-06, True, False, False, 0, 0): 0.759,
    ('gn', 'resident', (32, 32, 32, 128), 128, 32, 1e-06, True, False, False, 0, 0): 0.448,
    ('gn', 'resident', (32, 32, 32, 256), 128, 32, 1e-06, True, False, False, 0, 0): 0.302,
    ('gn', 'resident', (32, 4, 4, 256), 0, 32, 1e-06, False, False, False, 0, 0): 0.469,
    ('gn', 'resident', (32, 4, 4, 256), 0, 32, 1e-06, True, False, False, 0, 0): 0.621,
    ('gn', 'resident', (32, 4, 4, 256), 256, 32, 1e-06, True, False, False, 0, 0): 0.481,
    ('gn', 'resident', (32, 8, 8, 256), 0, 32, 1e-06, True, False, False, 0, 0): 0.605,
    ('gn', 'resident', (32, 8, 8, 256), 256, 32, 1e-06, True, False, False, 0, 0): 0.405,
    ('gn', 'resident', (32, 8, 8, 768), 0, 32, 1e-05, False, False, False, 0, 0): 0.579,
    ('gn', 'resident', (32, 8, 8, 768), 0, 32, 1e-05, True, False, False, 0, 0): 0.58,
    ('gn', 'resident', (32, 8, 8, 768), 768, 32, 1e-05, True, False, False, 0, 0): 0.412,
}

CASE_SET = set(CASES)


def _cx(xs, Cout, k, kid, stride=1, pad=None, pad_br=None, ups=0, res=False, variant=0):
    """An EXTRA conv row (bias, no addvec, no statistics, default tuning) that must select kernel `kid`."""
    return ("conv2d", xs, 0, Cout, k, False, stride, k // 2 if pad is None else pad, pad_br, ups, not res, "-", res, False, 0, False,
            False, None, variant, 0, "default", kid)


# Every conv kernel instance the forward dispatcher can select: conv_igemm_kernel<MB, NB, 32, PMAX> (MB * 1000 + NB * 100 + PMAX:
# 1 x 8 for Cout % 128 == 0, 2 x 4 with variant 1, 1 x 2 otherwise; PMAX 6 / 9 / 0 by the halo size), conv_pipe_kernel (10000 k +
# NB * 100 + PMAX: NB 2 or 4, PMAX 4 only for 3x3 at NB 4), conv1x1_stream_kernel, conv_stem_kernel, conv_ws_kernel<16 | 32>,
# conv_ws8_kernel without / with the fused GroupNorm output, conv_sm_kernel<log2 OW, 8, MT> (OW 4 | 8, MT 32 | 64),
# conv1x1_rw_kernel<NCH, R, RES> (NCH = K / 128 <= 4), conv1x1_rw8_kernel<NK, RES> (K = 384 / 512 / 576) and conv_head_kernel.
ALL_CONV_KERNEL_IDS = ({1800, 1806, 1809, 2400, 2406, 2409, 1200, 1206, 1209, 10206, 10406, 30206, 30404, 30406, 200000, 300000,
                        400016, 400032, 400008, 400009, 450432, 450464, 450832, 450864, 600000}
                       | {500000 + n * 1000 + (6 if n > 3 else 3) * 10 + r for n in range(1, 5) for r in (0, 1)}
                       | {550000 + nk * 10 + r for nk in (6, 8, 9) for r in (0, 1)})

# Forward kernel instances the programs never launch (conv rows: the kernel id they must select, last)
EXTRA = [
    _cx((3, 4, 4, 96), 128, 1, 1806, ups=1),                               # conv_igemm_kernel: Cin % 64 != 0 leaves conv_pipe
    _cx((3, 4, 4, 96), 128, 3, 1809),
    _cx((3, 8, 8, 96), 128, 3, 1800, stride=2, pad=0, pad_br=1),
    _cx((3, 4, 4, 64), 96, 1, 1206, ups=1),                                # Cout % 128 != 0: 32-cout tiles
    _cx((3, 4, 4, 64), 96, 3, 1209),
    _cx((3, 8, 8, 64), 96, 3, 1200, stride=2, pad=0, pad_br=1),
    _cx((5, 16, 16, 128), 128, 3, 2406, variant=1),                        # variant 1 skips the pipelined kernels
    _cx((3, 4, 4, 128), 128, 3, 2409, variant=1),
    _cx((3, 8, 8, 128), 128, 3, 2400, stride=2, pad=0, pad_br=1, variant=1),
    _cx((3, 4, 4, 64), 64, 1, 10206, ups=1),                               # conv_pipe 1x1 (nearest-upsampled input)
    _cx((1, 64, 64, 64), 512, 1, 10406, ups=1),
    _cx((1, 64, 64, 64), 512, 3, 30404, ups=1),                            # conv_pipe 3x3, 128-pixel tiles, two staging sets
    _cx((512, 4, 4, 64), 1024, 3, 30406),
    _cx((32, 32, 32, 128), 128, 1, 501031, res=True),                      # conv1x1_rw_kernel with the residual
    _cx((32, 32, 32, 512), 128, 1, 504061, res=True),
    ("linear", 8192, 256, 512, 0, 3, True, "tiled", 1),                   # P > 4096: the tiled conv path
    ("attention", 4, 256, 256, 2, True, True, "attention_kernel<128>"),
    ("attention", 4, 128, 256, 4, True, True, "attention_kernel<64>"),      # T % 256 != 0: the generic 64-wide kernel
    ("attention_proj", 5, 256, 256, 1, True),                              # attention256_kernel<true>
    ("nhwc_bf16_to_nchw_f32", (5, 16, 24, 40)),                            # layout copy and output stage: launched by the
    ("quantize_u8", (100, 3, 64, 64), 1, False),                           # generation scripts after the recorded programs
    ("quantize_u8", (7, 3, 32, 32), 0, True),
]
ATTN_KERNELS = {"attention_kernel<64>", "attention_kernel<128>", "attention_kernel<256>", "attention64", "attention256<false>"}


def _rows(op):
    return sorted({r for r in CASES if r[0] == op} | {r for r in EXTRA if r[0] == op}, key=repr)


def _id(r):
    return "-".join(str(v).replace(" ", "") for v in r[1:])


def _seed(r):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(r).encode()))


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    return o


def bf(t):
    return t.to(torch.bfloat16)


def rnd(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, device=DEV) * scale


class _tuned:
    def __init__(self, ops, tuning):
        self.cm = ops.throughput_tuning() if tuning == "throughput" else None

    def __enter__(self):
        if self.cm:
            self.cm.__enter__()

    def __exit__(self, *e):
        if self.cm:
            self.cm.__exit__(*e)


@pytest.mark.gpu
@pytest.mark.parametrize("program", sorted(PROGRAMS))
def test_census_is_covered(ops, program):
    import forward_census
    ops.device_check()
    rows, cond, unknown = forward_census.record(ops, program)
    assert not unknown, f"{program}: ops functions called outside a backward that are neither launch ops nor allowed: {unknown}"
    assert rows, f"{program}: nothing recorded"
    missing = sorted((r for r in rows if not _covered(r)), key=repr)
    assert not missing, f"{program}: forward launches not in CASES (add them): {missing}"
    for r, c in cond.items():
        assert c <= COND[r] * 1.5 + 1e-3, f"{program}: |mean|/std {c} of {r} above the recorded {COND[r]}"
    assert not [r for r in rows if r[0] == "linear" and r[-1] != 1], "a forward linear split K"


def _covered(r):
    """A census row is in CASES; a throughput-tuned conv row also when CASES holds it under the default tuning with the same
    kernel id (the table keeps one of two rows that run the same kernel on the same shapes)."""
    return r in CASE_SET or (r[0] == "conv2d" and r[-2] == "throughput" and r[:-2] + ("default", r[-1]) in CASE_SET)


def conv_kernel_names(rows):
    """bench.kernel_name of the kernel each conv row runs (400009: conv_ws8_kernel writing the fused GroupNorm output)."""
    import bench
    return {bench.kernel_name(400009 if (r[-1] == 400008 and r[17] is not None and r[17][3]) else r[-1]) for r in rows if r[0] == "conv2d"}


def test_extra_conv_rows_select_their_kernel(ops):
    """Host-side query (no launch): every EXTRA conv row selects the kernel id it names, and every CASES conv row the one
    the census recorded, under its tuning."""
    for r in [r for r in EXTRA + CASES if r[0] == "conv2d"]:
        assert forward_census.conv_kernel_id(ops, r) == r[-1], r


PLAN_QUERIES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_queries.json")


def conv_plan_queries(ops, r):
    """The host-side queries that read the forward conv selection besides the kernel id: GroupNorm statistics partials per
    image, the fused GroupNorm output (8 channels per group) in place of / next to the raw output, and the norm1 + 1x1
    shortcut fusion with 32 groups."""
    q = forward_census.conv_query
    fuse = dict(gn_groups=r[3] // 8)
    return [q(ops, r, "dxmi_conv2d_gn_stats_partials"),
            q(ops, r, "dxmi_conv2d_gn_fuse_supported", gn_flags=2, **fuse),
            q(ops, r, "dxmi_conv2d_gn_fuse_supported", gn_flags=0, **fuse),
            q(ops, r, "dxmi_groupnorm_silu_shortcut_supported", 32)]


def test_conv_rows_plan_queries(ops):
    """Host-side queries (no launch): every CASES + EXTRA conv row answers conv_plan_queries as recorded in
    golden/conv_plan_queries.json (rows not listed there answer all zeros)."""
    with open(PLAN_QUERIES) as f:
        want = json.load(f)
    got = {}
    for r in [r for r in EXTRA + CASES if r[0] == "conv2d"]:
        v = conv_plan_queries(ops, r)
        if any(v):
            got[repr(r)] = v
    assert got == want


@pytest.mark.parametrize("Cout", [4224, 8192])
def test_wide_1x1_reports_the_kernel_that_runs(ops, Cout):
    """1x1, K = 256, Cout / 128 > 32: beyond conv1x1_rw_kernel's 32 cout tiles, so the query names conv1x1_stream_kernel, which
    is what dxmi_conv2d_fwd launches."""
    assert forward_census.conv_kernel_id(ops, _cx((32, 32, 32, 256), Cout, 1, 200000)) == 200000


@pytest.mark.parametrize("hw", [4, 8])
def test_stats_request_on_small_maps_is_refused(ops, hw):
    """gn_stats on a 3x3 conv over 8x8 (conv_ws8_kernel) or 4x4 maps (conv_sm_kernel): neither kernel writes GroupNorm
    statistics, so dxmi_conv2d_fwd refuses the request before any launch (host-side: no device memory)."""
    C = 128 if hw == 8 else 256
    r = _cx((2, hw, hw, C), C, 3, 400008 if hw == 8 else 450432)
    assert forward_census.conv_kernel_id(ops, r) == r[-1]
    assert forward_census.conv_query(ops, r, "dxmi_conv2d_gn_stats_partials") == 0
    assert forward_census.conv_query(ops, r, "dxmi_conv2d_kernel_id", gn_stats=16) == -1      # DXMI_EINVAL: nothing to launch
    assert forward_census.conv_query(ops, r, "dxmi_conv2d_fwd", None, gn_stats=16) == -1
    assert "does not emit GroupNorm block statistics" in ops.load().dxmi_last_error().decode()


def test_table_reaches_every_conv_kernel():
    """CASES + EXTRA launch every conv kernel instance the forward dispatcher (conv_select and the *_select functions it
    tries) can select."""
    import bench
    assert conv_kernel_names(CASES + EXTRA) == {bench.kernel_name(k) for k in ALL_CONV_KERNEL_IDS}


def test_table_reaches_every_attention_kernel_linear_form_and_groupnorm_path():
    rows = set(CASES) | set(EXTRA)
    assert {r[-1] for r in rows if r[0] == "attention"} == ATTN_KERNELS
    assert {"attention_proj", "attn_block", "block_stats", "fold_stats", "gn_bs2gen"} <= {r[0] for r in rows}
    assert {r[7] for r in rows if r[0] == "linear"} == {"small", "tiled"}
    assert {r[1] for r in rows if r[0] == "gn"} == {"resident", "apply", "generic"}


# ------------------------------------------------------------------------------------------ conv
def _conv_inputs(ops, r, g):
    (_, xs, c1, Cout, k, k27, stride, pad, pad_br, ups, has_bias, addvec, has_res, has_mask, act, nchw, want_stats, fuse, variant,
     P, tuning, kid) = r
    N = xs[0]
    if k27:
        x0 = rnd(g, *xs)                                            # NCHW fp32 image; the kernel stages it as bf16
        xc = bf(x0).permute(0, 2, 3, 1)
        x1, Cin = None, 3
    else:
        x0 = bf(rnd(g, *xs))
        x1 = bf(rnd(g, *xs[:3], c1, scale=2.0)) if c1 else None
        xc = torch.cat([x0, x1], 3) if c1 else x0
        Cin = xs[3] + c1
    W = rnd(g, Cout, Cin, k, k, scale=(Cin * k * k) ** -0.5)
    pw = ops.pack_conv_weight(W, k27=k27)
    bias = rnd(g, Cout, scale=0.1) if has_bias else None
    av, avx = None, None
    if addvec == "shared":
        av = rnd(g, Cout, scale=0.3)
        avx = av[None].expand(N, Cout)
    elif addvec == "image":
        full = rnd(g, N, 3 * Cout, scale=0.3)                       # a row-strided slice, as the models' per-layer temb rows
        av = avx = full[:, Cout:2 * Cout]
    IH, IW = (xs[2], xs[3]) if k27 else (xs[1], xs[2])
    VH, VW = (2 * IH, 2 * IW) if ups else (IH, IW)
    pb = pad if pad_br is None else pad_br
    OH, OW = (VH + pad + pb - k) // stride + 1, (VW + pad + pb - k) // stride + 1
    res = bf(rnd(g, N, OH, OW, Cout)) if has_res else None
    return x0, x1, xc, W, pw, bias, av, avx, res


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("conv2d"), ids=_id)
def test_conv_fwd(ops, r):
    """Output element by element (depth Cin k k + 3, activation, one bf16 store), the selected kernel id, the block statistics
    of the stored output (per image and channel pair) and the fused GroupNorm output."""
    (_, xs, c1, Cout, k, k27, stride, pad, pad_br, ups, has_bias, addvec, has_res, has_mask, act, nchw, want_stats, fuse, variant,
     P, tuning, kid) = r
    assert not has_mask
    g = _seed(r)
    x0, x1, xc, W, pw, bias, av, avx, res = _conv_inputs(ops, r, g)
    Cin = xc.shape[3]
    kw = dict(in1=x1, bias=bias, addvec=av, residual=res, stride=stride, pad=pad, pad_br=pad_br, upsample=ups, act=act,
              out_nchw_f32=nchw, variant=variant, want_stats=want_stats)
    gamma = beta = None
    if fuse is not None:
        groups, silu, keep_raw = fuse[:3]
        gamma, beta = 1 + 0.3 * rnd(g, Cout), 0.3 * rnd(g, Cout)
        kw["fuse_gn"] = (gamma, beta, groups, 1e-6, silu, keep_raw)
    seen = []
    orig_fold = ops.fold_stats

    def fold(st, group=32):
        seen.append(st.P)
        return orig_fold(st, group)

    got_kid = []

    class Probe(ops.OpProfiler):
        def bracket(self, cls, name, flops, nbytes, fn):
            return fn()

        def launch_conv(self, d):
            import ctypes
            got_kid.append(int(ops.load().dxmi_conv2d_kernel_id(ctypes.byref(d))))
            ops.check(ops.load().dxmi_conv2d_fwd(ctypes.byref(d), ops._stream()), "dxmi_conv2d_fwd")

    old_prof, ops.PROFILER, ops.fold_stats = ops.PROFILER, Probe(), fold
    try:
        with _tuned(ops, tuning):
            res_ = ops.conv2d(x0, pw, **kw)
    finally:
        ops.PROFILER, ops.fold_stats = old_prof, orig_fold
    assert got_kid == [kid], f"selected kernel {got_kid} != census {kid}"
    out, st, y = res_, None, None
    if fuse is not None:
        out, y = res_
    elif want_stats:
        out, st = res_
    cr = conv_call_ref(x0, W, x1, bias, av, res, act=act, stride=stride, pad=pad, pad_br=pad_br, upsample=ups, out_nchw_f32=nchw)
    assert cr.K == (27 if k27 else Cin * k * k)
    name = f"conv2d[{r[-1]}]"
    if out is not None:
        CHECK.within(name, out, cr.ref, cr.bound)
    if st is not None:
        assert st.P == P
        S, Sa = stats_ref(out)
        HW = out.shape[1] * out.shape[2]
        P0 = seen[0] if seen else st.P
        c = stats_depth(HW, P0, fold_passes(P0))
        CHECK.fp32("block_stats[conv]", st.buf.double().sum(1), S, Sa, c)
    if y is not None:
        groups, silu = fuse[0], fuse[1]
        if out is not None:                                        # the kept raw tensor is what the epilogue normalised
            yo, parts = gn_ref(out, gamma, beta, groups, 1e-6, silu)
            bnd = gn_bound(yo, parts, gamma, beta, out.shape[1] * out.shape[2] * Cout // groups, silu)
        else:
            yo, parts = gn_ref(cr.ref, gamma, beta, groups, 1e-6, silu)
            bnd = gn_fused_bound(yo, parts, gamma, beta, cr.ref.shape[1] * cr.ref.shape[2] * Cout // groups, silu, cr.dh())
        CHECK.within("conv2d_fused_gn", y, yo, bnd)


# ------------------------------------------------------------------------------------------ GroupNorm
_gn_input = gn_input                    # moved to forward_bounds.py (the edge-case suite builds its inputs the same way)
_block_stats_tensor = block_stats_tensor


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("gn"), ids=_id)
def test_groupnorm_fwd(ops, r):
    """GroupNorm(+FiLM)(+SiLU) on the path the census saw (resident / streaming apply with P partials / generic), both concat
    sources, inputs with a realistic mean offset; bound with the conditioning term (mean^2 + var) / (var + eps) and eps."""
    _, path, xs, c1, groups, eps, silu, has_ss, saved, P0, P1 = r
    N, H, W, C0 = xs
    C = C0 + c1
    g = _seed(r)
    cond = max(MIN_COND, COND_MULT * COND.get(r, 0.0))
    xc = _gn_input(g, N, H, W, C, cond, groups)
    x0 = xc[..., :C0].contiguous()
    x1 = xc[..., C0:].contiguous() if c1 else None
    gamma, beta = 1 + 0.3 * rnd(g, C), 0.3 * rnd(g, C)
    ss = (0.3 * rnd(g, N, 3 * C))[:, C // 2: C // 2 + 2 * C] if has_ss else None
    st0 = st1 = None
    if path == "apply":
        st0 = ops.BlockStats(_block_stats_tensor(x0, P0), P0)
        st1 = ops.BlockStats(_block_stats_tensor(x1, P1), P1) if c1 else None
    else:
        assert path in ("generic", "resident")
    gn_fwd_checked(ops, path, x0, gamma, beta, in1=x1, groups=groups, eps=eps, silu=silu, scale_shift=ss, saved=[] if saved else None,
                   st0=st0, st1=st1, cond=cond, check=CHECK)


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("block_stats"), ids=_id)
def test_block_stats(ops, r):
    _, xs, P = r
    g = _seed(r)
    x = _gn_input(g, *xs, MIN_COND)
    seen = []
    orig = ops.fold_stats
    ops.fold_stats = lambda st, group=32: (seen.append(st.P), orig(st, group))[1]
    try:
        st = ops.block_stats(x)
    finally:
        ops.fold_stats = orig
    S, Sa = stats_ref(x)
    assert seen == ([P] if P > 8 else [])
    CHECK.fp32("block_stats", st.buf.double().sum(1), S, Sa, stats_depth(xs[1] * xs[2], P, fold_passes(P)))


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("fold_stats"), ids=_id)
def test_fold_stats(ops, r):
    """Each folded partial is the fp32 sum of `group` consecutive partials, in order: element-wise, depth group + 1."""
    _, N, P, C, group = r
    g = _seed(r)
    buf = (rnd(g, N, P, C // 2, 2) + 3.0).contiguous()
    st = ops.fold_stats(ops.BlockStats(buf, P), group)
    b = buf.double()
    PG = -(-P // group)
    pad = torch.zeros(N, PG * group - P, C // 2, 2, dtype=torch.float64, device=DEV)
    bb = torch.cat([b, pad], 1).reshape(N, PG, group, C // 2, 2)
    ref, A = bb.sum(2), bb.abs().sum(2)
    while ref.shape[1] > ops.MAX_APPLY_PARTIALS:
        PG2 = -(-ref.shape[1] // group)
        pad = torch.zeros(N, PG2 * group - ref.shape[1], C // 2, 2, dtype=torch.float64, device=DEV)
        ref = torch.cat([ref, pad], 1).reshape(N, PG2, group, C // 2, 2).sum(2)
        A = torch.cat([A, pad], 1).reshape(N, PG2, group, C // 2, 2).sum(2)
    CHECK.fp32("fold_stats", st.buf, ref, A, 2 * group + 2)


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("gn_bs2gen"), ids=_id)
def test_gn_blockstats_to_generic(ops, r):
    """The converted statistics drive groupnorm_generic_bwd(fwd_stats=...): its dx must match the fp64 backward as with the
    statistics the backward computes itself (tests/backward_bounds.py bound)."""
    _, N, HW, C0, C1, groups, P0, P1 = r
    H = W = int(round(HW ** 0.5))
    g = _seed(r)
    C = C0 + C1
    xc = _gn_input(g, N, H, W, C, 2.0, groups)
    x0 = xc[..., :C0].contiguous()
    x1 = xc[..., C0:].contiguous() if C1 else None
    st0 = ops.BlockStats(_block_stats_tensor(x0, P0), P0)
    st1 = ops.BlockStats(_block_stats_tensor(x1, P1), P1) if C1 else None
    fs = ops.gn_blockstats_to_generic(st0, st1, N, HW, C0, C1, groups)
    dy = bf(rnd(g, N, H, W, C))
    gamma, beta = 1 + 0.3 * rnd(g, C), 0.3 * rnd(g, C)
    dx0, dx1, _, _, _ = ops.groupnorm_generic_bwd(x0, dy, gamma, beta, in1=x1, groups=groups, eps=1e-6, silu=True, fwd_stats=fs)
    (rdx, _, _, _), (Adx, _, _, _) = groupnorm_bwd_ref(xc, dy, gamma, beta, groups, 1e-6, True)
    dx = torch.cat([dx0, dx1], 3) if C1 else dx0
    CHECK.bf16("gn_blockstats_to_generic[bwd dx]", dx, rdx, Adx, HW * C // groups + 16)


# ------------------------------------------------------------------------------------------ linear
@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("linear"), ids=_id)
def test_linear_fwd(ops, r):
    _, P, K, M, pre, post, has_bias, form, S = r
    assert S == 1
    g = _seed(r)
    x = rnd(g, P, K)
    W = rnd(g, M, K, scale=K ** -0.5)
    bias = rnd(g, M, scale=0.1) if has_bias else None
    got = ops.linear(x, ops.pack_conv_weight(W), bias, pre_act=pre, post_act=post)
    ref, bound = linear_ref(x, W, bias, pre, post)
    CHECK.within(f"linear[{form}]", got, ref, bound)


# ------------------------------------------------------------------------------------------ attention
def _attn_check(name, got, lse, qkv, heads, scale):
    N, T, C3 = qkv.shape
    o, lse2, smag, bound = attn_elem_bound(qkv, heads, scale)
    CHECK.blocks(name, attn_blocks(got, heads), attn_blocks(o, heads), 8 * U16, 3)
    CHECK.within(name + "_elem", got, o, bound)
    if lse is not None:
        CHECK.within(name + "_lse2", lse, lse2, lse_bound(lse2, smag, C3 // 3 // heads, T))
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("attention"), ids=_id)
def test_attention_fwd(ops, r):
    _, N, T, C, heads, want_lse, has_lse, kern = r
    g = _seed(r)
    qkv = bf(rnd(g, N, T, 3 * C))
    scale = (C // heads) ** -0.5
    lse = None
    if want_lse:
        got, lse = ops.attention(qkv, heads, scale, want_lse=True)
        assert (lse is not None) == has_lse
    else:
        got = ops.attention(qkv, heads, scale)
    _attn_check(f"attention[{kern}]", got, lse, qkv, heads, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("attention_proj"), ids=_id)
def test_attention_proj(ops, r):
    """x + proj_out(attention(qkv)) + bias: rel-L2 per (image, 128-row block) within 8 u16 of the fp64 chain."""
    _, N, T, C, heads, want_stats = r
    g = _seed(r)
    qkv = bf(rnd(g, N, T, 3 * C))
    x = bf(rnd(g, N, T, C))
    Wp = rnd(g, C, C, scale=C ** -0.5)
    bias = rnd(g, C, scale=0.1)
    scale = (C // heads) ** -0.5
    res = ops.attention_proj(qkv, ops.pack_attn_proj_weight(Wp), bias, x, heads, scale, want_stats=want_stats)
    got, st = res if want_stats else (res, None)
    o, _, _ = attention_ref(qkv, heads, scale)
    ref = x.double() + o @ bf(Wp).double().T + bias.double()
    CHECK.blocks("attention_proj", attn_blocks(got, 1), attn_blocks(ref, 1), 8 * U16, 3)
    if st is not None:
        S, Sa = stats_ref(got.view(N, 16, T // 16, C))
        CHECK.fp32("block_stats[attention_proj]", st.buf.double().sum(1), S, Sa, stats_depth(T, st.P, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("attn_block"), ids=_id)
def test_attn_block(ops, r):
    """x + proj(attention(q, k, v of GroupNorm(x))) with folded weights: rel-L2 per (image, 128-row block) within 8 u16 of the
    fp64 chain of the unfolded block."""
    _, xs, P, want_stats = r
    N, C = xs[0], xs[-1]
    T = 1
    for v in xs[1:-1]:
        T *= v
    g = _seed(r)
    x = _gn_input(g, N, 16, T // 16, C, MIN_COND).reshape(xs)
    st = ops.BlockStats(_block_stats_tensor(x.reshape(N, 16, T // 16, C), P), P)
    gamma, beta = 1 + 0.3 * rnd(g, C), 0.3 * rnd(g, C)
    ws = [rnd(g, C, C, scale=C ** -0.5) for _ in range(4)]
    bs = [rnd(g, C, scale=0.1) for _ in range(3)]
    scale = C ** -0.5
    packed = ops.attn_block_pack(ws[0], bs[0], ws[1], ws[2], bs[1], ws[3], bs[2], scale)
    res = ops.attn_block(x, st, gamma, beta, packed, eps=1e-6, want_stats=want_stats)
    got, st_out = res if want_stats else (res, None)
    xd = x.double().reshape(N, T, C)
    hn, _ = gn_ref(x.reshape(N, 16, T // 16, C), gamma, beta, 32, 1e-6, False)
    hn = hn.reshape(N, T, C)
    q = hn @ ws[0].double().T + bs[0].double()
    k = hn @ ws[1].double().T
    v = hn @ ws[2].double().T + bs[1].double()
    p = torch.softmax(scale * q @ k.transpose(1, 2), -1)
    ref = xd + (p @ v) @ ws[3].double().T + bs[2].double()
    CHECK.blocks("attn_block", attn_blocks(got.reshape(N, T, C), 1), attn_blocks(ref, 1), 8 * U16, 3)
    if st_out is not None:
        S, Sa = stats_ref(got.reshape(N, 16, T // 16, C))
        CHECK.fp32("block_stats[attn_block]", st_out.buf.double().sum(1), S, Sa, stats_depth(T, st_out.P, 0))


# ------------------------------------------------------------------------------------------ small ops
@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("timestep_embedding"), ids=_id)
def test_timestep_embedding(ops, r):
    """sin / cos of t * freq: the fp32 argument carries 4 u32 |t freq| (the frequency's own expf and the product), the
    functions a few ulps."""
    _, n, dim, order, max_period = r
    t = torch.linspace(0, 999, n, device=DEV)
    got = ops.timestep_embedding(t, dim, order=order, max_period=max_period)
    half = dim // 2
    i = torch.arange(half, device=DEV, dtype=torch.float64)
    denom = (half - 1) if order == 0 else half
    import math
    arg = t.double()[:, None] * torch.exp(-math.log(max_period) * i / denom)[None]
    s, c = torch.sin(arg), torch.cos(arg)
    ref = torch.cat([s, c], 1) if order == 0 else torch.cat([c, s], 1)
    a2 = torch.cat([arg, arg], 1).abs()
    CHECK.within("timestep_embedding", got, ref, 8 * U32 * a2 + 4 * U32)


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("upsample2x"), ids=_id)
def test_upsample2x(ops, r):
    x = bf(rnd(_seed(r), *r[1]))
    assert torch.equal(ops.upsample2x(x), x.repeat_interleave(2, 1).repeat_interleave(2, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("pool_act"), ids=_id)
def test_pool_act(ops, r):
    _, xs, pool, act = r
    x = bf(rnd(_seed(r), *xs))
    CHECK.within("pool_act", ops.pool_act(x, pool, act), *pool_act_ref(x, pool, act))


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("value_head"), ids=_id)
def test_value_head(ops, r):
    """relu -> sum over pixels -> dot(w) + b (-> out_w y + out_b): fp32 depth HW + C + 4."""
    _, xs, has_out = r
    g = _seed(r)
    x = bf(rnd(g, *xs))
    N, H, W, C = xs
    w, b = rnd(g, C, scale=C ** -0.5), rnd(g, 1)
    ow, ob = (rnd(g, 1), rnd(g, 1)) if has_out else (None, None)
    got = ops.value_head(x, w, b, ow, ob)
    s = x.double().clamp_min(0).sum((1, 2))
    ref = s @ w.double() + b.double()
    A = s @ w.double().abs() + b.double().abs()
    if has_out:
        ref, A = ref * ow.double() + ob.double(), A * ow.double().abs() + ob.double().abs()
    CHECK.fp32("value_head", got.reshape(-1), ref, A, H * W + C + 4)


# ------------------------------------------------------------------------------------------ non-network launches of a step
@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("dropout"), ids=_id)
def test_dropout_fwd(ops, r):
    """Kept set bit-equal to the hash restatement; kept values bf16(x / (1 - p)) of the fp64 quotient (either neighbour where
    the quotient is within 4 u32 of a rounding midpoint).  The backward replay is in test_hip_backward_shapes.py."""
    _, shape, p, on_dev = r
    assert not on_dev
    x = bf(rnd(_seed(r), *shape))
    seed = ops.dropout_site_seed(zlib.crc32(repr(r).encode()), 3)
    y = ops.dropout(x, p, seed)
    keep, ref, tie = dropout_ref(x, p, seed)
    assert torch.equal((y != 0) | (x == 0), keep | (x == 0)), "kept set differs from the hash"
    assert not bool(((y != ref) & ~tie).any()) and bool(((y.double() - ref.double()).abs() <= 2 * U16 * ref.double().abs()).all())
    CHECK._note("dropout[mismatches]", 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("edm_dsm_prep") + _rows("edm_dsm_loss_fwd"), ids=_id)
def test_edm_dsm_fwd(ops, r):
    """edm_dsm_prep and the per-sample DSM terms at the recorded batch against the fp64 expressions of
    test_hip_edm_dsm.py::test_dsm_kernels_vs_fp64 (operands, scalings64, weights64 imported from there), with the bounds derived
    in forward_bounds (scaled_input_ref, log_sigma_t, dsm_error_terms, dsm_loss_fwd_bound)."""
    from test_hip_edm_dsm import operands, scalings64, weights64
    shape = r[1]
    N, CHW = shape[0], shape[1] * shape[2] * shape[3]
    x0, noise, F_, sig = [t.to(DEV) for t in operands(N, CHW, zlib.crc32(repr(r).encode()) % 1000)]
    v4 = lambda t: t.view(shape).contiguous()
    if r[0] == "edm_dsm_prep":
        x_in, t = ops.edm_dsm_prep(v4(x0), v4(noise), sig)
        ref, A = scaled_input_ref(x0, sig, noise)
        CHECK.fp32("edm_dsm_prep_x", x_in.view(N, CHW), ref, A, 16)
        CHECK.within("edm_dsm_prep_t", t, *log_sigma_t(sig))
        return
    _, _, ws, distill = r
    xs, mse = ops.edm_dsm_loss_fwd(v4(F_), v4(x0), v4(noise), sig, ws, distillation=distill)
    e, Me, _ = dsm_error_terms(F_, x0, noise, sig, scalings64(sig, distill=distill))
    CHECK.within("edm_dsm_loss_fwd_xs", xs, *dsm_loss_fwd_bound(e, Me))
    CHECK.within("edm_dsm_loss_fwd_mse", mse, *dsm_loss_fwd_bound(e, Me, weights64(ws, sig)))


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("td_gather_cost"), ids=_id)
def test_td_gather_cost(ops, r):
    """[next_state | state] gathered bit for bit from the trajectory block; running cost mean_CHW (x' - x)^2 / (2 beta): a sum
    of depth CHW of fp32 squares of fp32 differences."""
    _, B, CHW, has = r
    assert has == ("next_rows",)
    g = _seed(r)
    rows = 11 * B
    traj = rnd(g, rows, CHW)
    srows = torch.randperm(rows - B, generator=g, device=DEV)[:B].contiguous()
    nrows = srows + B
    beta = torch.full((1,), 0.37, device=DEV)
    pair = torch.empty(2 * B, CHW, device=DEV)
    cost = ops.td_gather_cost(traj, srows, beta, next_rows=nrows, out_pair=pair)
    assert torch.equal(pair[:B], traj[nrows]) and torch.equal(pair[B:], traj[srows])
    CHECK.fp32("td_gather_cost", cost, *td_gather_cost_ref(traj[nrows], traj[srows], beta), CHW + 8)


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("td_loss"), ids=_id)
def test_td_loss_fwd(ops, r):
    check_td_loss(ops, CHECK, r)


def check_td_loss(ops, check, r):
    """d loss / d v (zeros in the target half) and the three logged means of one td_loss row against fp64 autograd: depth-B
    sums (shared with test_hip_backward_shapes.py, where td_loss is a row of the backward census too)."""
    _, B, has_extra = r
    g = _seed(r)
    v, cost = rnd(g, 2 * B), rnd(g, B).abs()
    extra = rnd(g, 1) if has_extra else None
    grad, logs = ops.td_loss(v, cost, extra)
    rg, rl, Ag, Al = td_loss_ref(v, cost, extra)
    assert torch.equal(grad[:B], torch.zeros_like(grad[:B]))
    check.fp32("td_loss_grad", grad, rg, Ag, 8)
    check.fp32("td_loss_logs", logs, rl, Al, B + 8)


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("var_step"), ids=_id)
def test_var_step(ops, r):
    """The VAR transition at the recorded batches, both associations of x' (assoc 1: the sampling loop, 0: the training step),
    per-sample schedule scalars all different: forward_bounds.var_step_ref."""
    _, shape, want_mean, want_control, assoc = r
    N, CHW = shape[0], shape[1] * shape[2] * shape[3]
    g = _seed(r)
    x, eps, z = rnd(g, *shape), rnd(g, *shape), rnd(g, *shape)
    xm, cm, sg = rnd(g, N).abs() + 0.5, -rnd(g, N).abs() - 0.1, torch.exp(rnd(g, N) * 0.3 - 1.0)
    got = dict(zip(("x_next", "mean", "control", "logp"),
                   ops.var_step(x, eps, z, xm, cm, sg, want_mean=want_mean, want_control=want_control, assoc=assoc)))
    assert (got["mean"] is not None) == want_mean and (got["control"] is not None) == want_control
    f = lambda t: t.view(N, CHW)
    for k, (ref, bound) in var_step_ref(f(x), f(eps), f(z), xm, cm, sg).items():
        if got[k] is not None:
            CHECK.within(f"var_step_{k}", got[k].view(ref.shape), ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("edm_step") + _rows("edm_precond"), ids=_id)
def test_edm_step_and_precond(ops, r):
    """The EDM transition and its preconditioning at the recorded batches, one sigma per sample over the whole ladder."""
    shape = r[1]
    N, CHW = shape[0], shape[1] * shape[2] * shape[3]
    g = _seed(r)
    f = lambda t: t.view(N, CHW)
    x = rnd(g, *shape)
    sigma = torch.exp(torch.linspace(-6.2, 4.38, N, device=DEV))          # 0.002 .. 80
    if r[0] == "edm_precond":
        x_in, t = ops.edm_precond(x, sigma)
        ref, A = scaled_input_ref(f(x), sigma)
        CHECK.fp32("edm_precond_x", f(x_in), ref, A, 16)
        CHECK.within("edm_precond_t", t, *log_sigma_t(sigma))
        return
    F_, z = rnd(g, *shape), rnd(g, *shape)
    sdn, sup = sigma * (0.2 + 0.6 * torch.rand(N, generator=g, device=DEV)), sigma * 0.3
    sample, mean = ops.edm_step(x, F_, z, sigma, sdn, sup)
    mu, smp, Am, As = edm_step_ref(f(x), f(F_), f(z), sigma, sdn, sup)
    CHECK.fp32("edm_step_mean", f(mean), mu, Am, 16)
    CHECK.fp32("edm_step_sample", f(sample), smp, As, 16)


def _stage_io(shape, g, names):
    """Seeded state / operand tensors of a sampler stage on the host (the references of the sampler tests take host tensors)."""
    t = {k: 1.5 * torch.randn(shape, generator=g) for k in ("x", "x2", "d")}
    t["F"] = 3.0 * torch.randn(shape, generator=g)             # c_out F + c_skip x lands on both sides of the +-1 clamp
    t["noise"] = torch.randn(shape, generator=g)
    t["ref"] = torch.rand(shape, generator=g) * 2 - 1
    t["mask"] = (torch.rand(shape, generator=g) > 0.5).float()
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("karras_stage"), ids=_id)
def test_karras_stage(ops, r):
    """dxmi_karras_stage with exactly the operands the sampler passed, at the recorded batch, against the fp64 restatement of
    test_hip_karras_sample.py (_row, _ref_stage, imported) with that test's bound: every output an fp32 expression of <= 8
    operations on table scalars, 16 u32 times the sum M of its absolute terms; clip on and off."""
    from test_hip_karras_sample import _ref_stage, _row
    _, mode, last, shape, has = r
    N = shape[0]
    for clip in (1.0, 0.0):
        g = torch.Generator().manual_seed(zlib.crc32(repr((r, clip)).encode()))
        tab = _row(g, mode, clip)
        h = _stage_io(shape, g, has)
        dev = {k: v.to(DEV).contiguous() for k, v in h.items()}
        outs = {k: torch.full(shape, float("nan"), device=DEV) for k in ("x_in", "out", "denoised") if k in has}
        t = torch.full((N,), float("nan"), device=DEV) if "t" in has else None
        ops.karras_stage(mode, last, tab.to(DEV), 1, dev["x"], x2=dev["x2"] if "x2" in has else None, d=dev["d"] if "d" in has else None,
                         model_out=dev["F"] if "model_out" in has else None, noise=dev["noise"] if "noise" in has else None,
                         x_in=outs.get("x_in"), t=t, out=outs.get("out"), denoised=outs.get("denoised"))
        got = {"x": dev["x"], "x2": dev["x2"], "d": dev["d"], **outs}
        want = _ref_stage(mode, last, tab[1], h["x"], h["x2"], h["d"], h["F"], h["noise"] if "noise" in has else None)
        assert set(want) - {"denoised"} <= set(got)
        for k, (w, M) in want.items():
            if k in got:
                CHECK.fp32(f"karras_stage[{mode}]_{k}", got[k], w.to(DEV), M.to(DEV), 16)
        if t is not None:
            assert torch.equal(t.cpu(), tab[1, ops.KT_T].expand(N))


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("cm_stage"), ids=_id)
def test_cm_stage(ops, r):
    """dxmi_cm_stage with exactly the operands the sampler / editing loop passed, at the recorded batch, against the fp64
    restatement of test_hip_cm_sample.py (_table, _ref_stage, imported) with that test's bound 16 u32 M (+ 136 u32 M_Q for the
    basis changes, which no recorded row uses); clip / output clamp on and off."""
    from models.cm.karras_diffusion import colour_basis, patch_basis
    from test_hip_cm_sample import _ref_stage, _table
    _, mode, edit, last, shape, has = r
    N = shape[0]
    Q = {ops.CM_EDIT_COLOUR: colour_basis(), ops.CM_EDIT_PATCH: patch_basis()}.get(edit)
    assert (Q is not None) == ("Q" in has)
    for clip, out_clamp in ((1.0, 1.0), (0.0, 0.0)):
        g = torch.Generator().manual_seed(zlib.crc32(repr((r, clip)).encode()))
        tab = _table(g, mode, last, clip, out_clamp)
        h = _stage_io(shape, g, has)
        dev = {k: v.to(DEV).contiguous() for k, v in h.items()}
        outs = {k: torch.full(shape, float("nan"), device=DEV) for k in ("x_in", "out", "denoised") if k in has}
        t = torch.full((N,), float("nan"), device=DEV) if "t" in has else None
        opt = lambda name, key: dev[key] if name in has else None
        ops.cm_stage(mode, last, tab.to(DEV), 1, dev["x"], edit=edit, Q=None if Q is None else Q.to(DEV), model_out=opt("model_out", "F"),
                     noise=opt("noise", "noise"), ref=opt("ref", "ref"), mask=opt("mask", "mask"), x_in=outs.get("x_in"), t=t,
                     out=outs.get("out"), denoised=outs.get("denoised"))
        got = {"x": dev["x"], **outs}
        want = _ref_stage(mode, edit, last, tab[1], Q, h["x"], h["F"], h["noise"] if "noise" in has else None, h["ref"], h["mask"])
        assert set(want) - {"denoised"} <= set(got)
        for k, (w, Me, Mq) in want.items():
            if k in got:
                CHECK.within(f"cm_stage[{mode},{edit}]_{k}", got[k], w.to(DEV), (16 * U32 * Me + 136 * U32 * Mq).to(DEV))
        if t is not None:
            assert torch.equal(t.cpu(), tab[1, ops.CT_T].expand(N))


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("gn_shortcut"), ids=_id)
def test_groupnorm_silu_shortcut(ops, r):
    """The fused norm1 + 1x1 shortcut kernel at the recorded shapes: y against the fp64 GroupNorm of the streaming-apply path
    (block statistics with the recorded partial counts), the shortcut against the fp64 1x1 conv of the same input."""
    _, xs, c1, Cout, groups, eps, silu, has_bias, P0, P1 = r
    N, H, W, C0 = xs
    C = C0 + c1
    g = _seed(r)
    xc = _gn_input(g, N, H, W, C, MIN_COND, groups)
    x0 = xc[..., :C0].contiguous()
    x1 = xc[..., C0:].contiguous() if c1 else None
    gamma, beta = 1 + 0.3 * rnd(g, C), 0.3 * rnd(g, C)
    Wt = rnd(g, Cout, C, 1, 1, scale=C ** -0.5)
    bias = rnd(g, Cout, scale=0.1) if has_bias else None
    st0 = ops.BlockStats(_block_stats_tensor(x0, P0), P0)
    st1 = ops.BlockStats(_block_stats_tensor(x1, P1), P1) if c1 else None
    res = ops.groupnorm_silu_shortcut(x0, gamma, beta, ops.pack_conv_weight(Wt), in1=x1, bias=bias, groups=groups, eps=eps, silu=silu,
                                      stats=(st0, st1))
    assert res is not None, "the census saw this shape launch the fused kernel"
    y, sc = res
    yo, parts = gn_ref(xc, gamma, beta, groups, eps, silu, None)
    CHECK.within("gn_shortcut_y", y, yo, gn_bound(yo, parts, gamma, beta, max(P0, P1) + C // groups // 2 + 2, silu))
    c = conv_call_ref(x0, Wt, x1, bias)
    assert c.K == C
    CHECK.within("gn_shortcut_conv", sc, c.ref, c.bound)


@pytest.mark.gpu
@pytest.mark.parametrize("r", _rows("var_gather_sched") + _rows("nhwc_bf16_to_nchw_f32") + _rows("quantize_u8"), ids=_id)
def test_gathers_and_layout_copies(ops, r):
    """The integer schedule gather, the layout copy and the output stage, bit-equal to stock torch (sigma = exp(log_betas): fp32
    expf against the fp64 exponential within 4 u32)."""
    g = _seed(r)
    if r[0] == "var_gather_sched":
        _, N, T = r
        t = torch.randint(-T, T, (N,), generator=g, device=DEV)                     # negative steps wrap as torch indexing does
        tabs = [rnd(g, T) for _ in range(4)]
        tau, xm, cm, sg = ops.var_gather_sched(t, *tabs)
        assert torch.equal(tau, tabs[0][t]) and torch.equal(xm, tabs[1][t]) and torch.equal(cm, tabs[2][t])
        ref = torch.exp(tabs[3][t].double())
        CHECK.fp32("var_gather_sched_sigma", sg, ref, ref, 4)
    elif r[0] == "nhwc_bf16_to_nchw_f32":
        x = bf(rnd(g, *r[1]))
        assert torch.equal(ops.nhwc_bf16_to_nchw_f32(x), x.float().permute(0, 3, 1, 2).contiguous())
    else:
        _, shape, mode, nhwc = r
        x = rnd(g, *shape) * 0.8
        if mode == 1:
            ref = ((x + 1) * 127.5).clamp(0, 255).to(torch.uint8)
        else:
            ref = (((x + 1) / 2).clamp(0, 1) * 255 + 0.5).clamp(0, 255).to(torch.uint8)
        got = ops.quantize_u8(x, mode=mode, nhwc=nhwc)
        assert torch.equal(got, ref.permute(0, 2, 3, 1).contiguous() if nhwc else ref)


def test_every_row_kind_has_a_test():
    """Host-side: the op kinds of CASES + EXTRA are exactly the kinds some test of this file parametrises over."""
    import re
    src = open(os.path.abspath(__file__)).read()
    tested = set(re.findall(r'_rows\("([a-z0-9_]+)"\)', src))
    assert {r[0] for r in CASES + EXTRA} == tested, {r[0] for r in CASES + EXTRA} ^ tested


@pytest.mark.gpu
def test_report():
    """Largest |err| / bound per op over the cases above (printed; run with -s)."""
    for k, v in CHECK.report().items():
        print(f"{k:48s} {v:.4f}")
