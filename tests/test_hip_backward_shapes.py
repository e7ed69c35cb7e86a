"""Every backward launch of the training programs against an fp64 reference, at the shapes the programs use.

CASES below is the census of the backward launches of one eager iteration of each program of backward_census.PROGRAMS
(tests/backward_census.py), each recorded under the tuning the program runs under:
    imagenet64    DxMI step on imagenet64_T10, per-GPU batch 16                 ops.throughput_tuning()
    cifar10       DxMI step on cifar10_T10 (U-Net and value net), batch 128     ops.throughput_tuning()
    edm_dsm_b16   DSM microbatch of the full-size EDM U-Net (TrainLoop), 16     default knobs
    edm_dsm_b32   the same at 32 images                                         default knobs
test_census_is_covered re-records each program and fails when it launches a shape the table does not hold, or calls an `ops`
function inside a backward that is neither a launch op nor on the census's allow-list (record or refuse).  Each row is then
checked on seeded inputs against stock torch in float64 on the device (F.unfold + matmul for convolutions and weight
gradients, softmax attention and F.group_norm under autograd, plain expressions for the element-wise ops), with the
element-wise bounds of tests/backward_bounds.py; none of this project's kernels takes part in a reference.  test_report
prints the largest |err| / bound seen per op; test_every_row_kind_has_a_test keeps the kinds of the table and of the tests equal.
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

from backward_bounds import (U16, U32, Checker, attention_bwd_checked, attention_bwd_ref, dropout_ref, dsm_loss_bwd_ref,
                             edm_step_bwd_ref, gn_bwd_checked, silu_bwd_ref, unfold_nhwc, value_head_bwd_ref, value_head_pgrad_ref,
                             var_step_bwd_ref, wgrad_checked, wgrad_depth, wgrad_ref)
from forward_bounds import FwdChecker, dsm_error_terms, linear_ref, pool_act_ref

DEV = "cuda:0"
CHECK = FwdChecker()              # Checker plus `within` (an explicit element-wise bound) for the forward kernels' rows

CASES = {
    'wgrad': [
        # (op, x NHWC, C1, dy NHWC, k, pad, stride, upsample, accumulate, with_bias)
        ('wgrad', (1, 4, 16, 192), 0, (1, 4, 16, 768), 1, 0, 1, 0, False, False),
        ('wgrad', (1, 4, 16, 768), 0, (1, 4, 16, 35712), 1, 0, 1, 0, False, False),
        ('wgrad', (1, 4, 16, 768), 0, (1, 4, 16, 768), 1, 0, 1, 0, False, False),
        ('wgrad', (1, 8, 16, 128), 0, (1, 8, 16, 512), 1, 0, 1, 0, False, False),
        ('wgrad', (1, 8, 16, 512), 0, (1, 8, 16, 4992), 1, 0, 1, 0, False, False),
        ('wgrad', (1, 8, 16, 512), 0, (1, 8, 16, 512), 1, 0, 1, 0, False, False),
        ('wgrad', (128, 16, 16, 128), 0, (128, 16, 16, 128), 3, 1, 1, 0, False, True),
        ('wgrad', (128, 16, 16, 128), 0, (128, 16, 16, 256), 1, 0, 1, 0, False, False),
        ('wgrad', (128, 16, 16, 128), 0, (128, 16, 16, 256), 1, 0, 1, 0, False, True),
        ('wgrad', (128, 16, 16, 128), 0, (128, 16, 16, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (128, 16, 16, 256), 0, (128, 16, 16, 256), 1, 0, 1, 0, False, True),
        ('wgrad', (128, 16, 16, 256), 0, (128, 16, 16, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (128, 16, 16, 256), 0, (128, 16, 16, 768), 1, 0, 1, 0, False, True),
        ('wgrad', (128, 16, 16, 256), 0, (128, 32, 32, 256), 3, 1, 1, 1, False, True),
        ('wgrad', (128, 16, 16, 256), 0, (128, 8, 8, 256), 3, 0, 2, 0, False, True),
        ('wgrad', (128, 16, 16, 256), 128, (128, 16, 16, 256), 1, 0, 1, 0, False, True),
        ('wgrad', (128, 16, 16, 256), 256, (128, 16, 16, 256), 1, 0, 1, 0, False, True),
        ('wgrad', (128, 16, 16, 384), 0, (128, 16, 16, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (128, 16, 16, 512), 0, (128, 16, 16, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (128, 32, 32, 128), 0, (128, 16, 16, 128), 3, 0, 2, 0, False, True),
        ('wgrad', (128, 32, 32, 128), 0, (128, 32, 32, 128), 1, 0, 1, 0, False, False),
        ('wgrad', (128, 32, 32, 128), 0, (128, 32, 32, 128), 3, 1, 1, 0, False, True),
        ('wgrad', (128, 32, 32, 128), 0, (128, 32, 32, 64), 3, 1, 1, 0, False, False),
        ('wgrad', (128, 32, 32, 128), 128, (128, 32, 32, 128), 1, 0, 1, 0, False, True),
        ('wgrad', (128, 32, 32, 256), 0, (128, 32, 32, 128), 3, 1, 1, 0, False, True),
        ('wgrad', (128, 32, 32, 256), 128, (128, 32, 32, 128), 1, 0, 1, 0, False, True),
        ('wgrad', (128, 32, 32, 384), 0, (128, 32, 32, 128), 3, 1, 1, 0, False, True),
        ('wgrad', (128, 32, 32, 64), 0, (128, 32, 32, 128), 1, 0, 1, 0, False, False),
        ('wgrad', (128, 4, 4, 256), 0, (128, 4, 4, 256), 1, 0, 1, 0, False, True),
        ('wgrad', (128, 4, 4, 256), 0, (128, 4, 4, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (128, 4, 4, 256), 0, (128, 4, 4, 768), 1, 0, 1, 0, False, True),
        ('wgrad', (128, 4, 4, 256), 0, (128, 8, 8, 256), 3, 1, 1, 1, False, True),
        ('wgrad', (128, 4, 4, 256), 256, (128, 4, 4, 256), 1, 0, 1, 0, False, True),
        ('wgrad', (128, 4, 4, 512), 0, (128, 4, 4, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (128, 8, 8, 256), 0, (128, 16, 16, 256), 3, 1, 1, 1, False, True),
        ('wgrad', (128, 8, 8, 256), 0, (128, 4, 4, 256), 3, 0, 2, 0, False, True),
        ('wgrad', (128, 8, 8, 256), 0, (128, 8, 8, 256), 1, 0, 1, 0, False, False),
        ('wgrad', (128, 8, 8, 256), 0, (128, 8, 8, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (128, 8, 8, 256), 256, (128, 8, 8, 256), 1, 0, 1, 0, False, True),
        ('wgrad', (128, 8, 8, 512), 0, (128, 8, 8, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 16, 16, 1152), 0, (16, 16, 16, 576), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 16, 16, 1344), 0, (16, 16, 16, 576), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 16, 16, 256), 0, (16, 16, 16, 256), 1, 0, 1, 0, False, False),
        ('wgrad', (16, 16, 16, 256), 0, (16, 16, 16, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 16, 16, 384), 0, (16, 16, 16, 384), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 16, 16, 384), 0, (16, 16, 16, 576), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 16, 16, 384), 0, (16, 16, 16, 576), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 16, 16, 576), 0, (16, 16, 16, 1728), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 16, 16, 576), 0, (16, 16, 16, 576), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 16, 16, 576), 0, (16, 16, 16, 576), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 16, 16, 576), 0, (16, 32, 32, 576), 3, 1, 1, 1, False, True),
        ('wgrad', (16, 16, 16, 576), 384, (16, 16, 16, 576), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 16, 16, 576), 576, (16, 16, 16, 576), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 16, 16, 768), 0, (16, 16, 16, 768), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 16, 16, 768), 576, (16, 16, 16, 576), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 16, 16, 960), 0, (16, 16, 16, 576), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 32, 32, 128), 0, (16, 32, 32, 128), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 32, 32, 128), 0, (16, 32, 32, 256), 1, 0, 1, 0, False, False),
        ('wgrad', (16, 32, 32, 128), 0, (16, 32, 32, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 32, 32, 192), 0, (16, 32, 32, 192), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 32, 32, 192), 0, (16, 32, 32, 384), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 32, 32, 192), 0, (16, 32, 32, 384), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 32, 32, 256), 0, (16, 32, 32, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 32, 32, 384), 0, (16, 32, 32, 1152), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 32, 32, 384), 0, (16, 32, 32, 384), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 32, 32, 384), 0, (16, 32, 32, 384), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 32, 32, 384), 0, (16, 64, 64, 384), 3, 1, 1, 1, False, True),
        ('wgrad', (16, 32, 32, 384), 192, (16, 32, 32, 384), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 32, 32, 384), 384, (16, 32, 32, 384), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 32, 32, 576), 0, (16, 32, 32, 384), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 32, 32, 576), 0, (16, 32, 32, 576), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 32, 32, 576), 384, (16, 32, 32, 384), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 32, 32, 768), 0, (16, 32, 32, 384), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 32, 32, 960), 0, (16, 32, 32, 384), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 64, 64, 128), 0, (16, 64, 64, 128), 1, 0, 1, 0, False, False),
        ('wgrad', (16, 64, 64, 128), 0, (16, 64, 64, 128), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 64, 64, 192), 0, (16, 64, 64, 192), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 64, 64, 192), 0, (16, 64, 64, 64), 3, 1, 1, 0, False, False),
        ('wgrad', (16, 64, 64, 192), 192, (16, 64, 64, 192), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 64, 64, 384), 0, (16, 64, 64, 192), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 64, 64, 384), 0, (16, 64, 64, 384), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 64, 64, 384), 192, (16, 64, 64, 192), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 64, 64, 576), 0, (16, 64, 64, 192), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 64, 64, 64), 0, (16, 64, 64, 128), 1, 0, 1, 0, False, False),
        ('wgrad', (16, 64, 64, 64), 0, (16, 64, 64, 192), 1, 0, 1, 0, False, False),
        ('wgrad', (16, 8, 8, 1344), 0, (16, 8, 8, 768), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 8, 8, 1536), 0, (16, 8, 8, 768), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 8, 8, 256), 0, (16, 8, 8, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 8, 8, 576), 0, (16, 8, 8, 576), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 8, 8, 576), 0, (16, 8, 8, 768), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 8, 8, 576), 0, (16, 8, 8, 768), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 8, 8, 768), 0, (16, 16, 16, 768), 3, 1, 1, 1, False, True),
        ('wgrad', (16, 8, 8, 768), 0, (16, 8, 8, 2304), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 8, 8, 768), 0, (16, 8, 8, 768), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 8, 8, 768), 0, (16, 8, 8, 768), 3, 1, 1, 0, False, True),
        ('wgrad', (16, 8, 8, 768), 576, (16, 8, 8, 768), 1, 0, 1, 0, False, True),
        ('wgrad', (16, 8, 8, 768), 768, (16, 8, 8, 768), 1, 0, 1, 0, False, True),
        ('wgrad', (256, 16, 16, 128), 0, (256, 16, 16, 128), 3, 1, 1, 0, False, True),
        ('wgrad', (256, 16, 16, 128), 0, (256, 16, 16, 256), 1, 0, 1, 0, False, False),
        ('wgrad', (256, 16, 16, 128), 0, (256, 16, 16, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (256, 16, 16, 256), 0, (256, 16, 16, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (256, 32, 32, 128), 0, (256, 32, 32, 128), 1, 0, 1, 0, False, False),
        ('wgrad', (256, 32, 32, 128), 0, (256, 32, 32, 128), 3, 1, 1, 0, False, True),
        ('wgrad', (256, 32, 32, 64), 0, (256, 32, 32, 128), 1, 0, 1, 0, False, False),
        ('wgrad', (256, 4, 4, 256), 0, (256, 4, 4, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (256, 8, 8, 256), 0, (256, 8, 8, 256), 1, 0, 1, 0, False, False),
        ('wgrad', (256, 8, 8, 256), 0, (256, 8, 8, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 16, 16, 1152), 0, (32, 16, 16, 576), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 16, 16, 1344), 0, (32, 16, 16, 576), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 16, 16, 256), 0, (32, 16, 16, 256), 1, 0, 1, 0, False, False),
        ('wgrad', (32, 16, 16, 256), 0, (32, 16, 16, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 16, 16, 384), 0, (32, 16, 16, 384), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 16, 16, 384), 0, (32, 16, 16, 576), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 16, 16, 384), 0, (32, 16, 16, 576), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 16, 16, 576), 0, (32, 16, 16, 1728), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 16, 16, 576), 0, (32, 16, 16, 576), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 16, 16, 576), 0, (32, 16, 16, 576), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 16, 16, 576), 0, (32, 32, 32, 576), 3, 1, 1, 1, False, True),
        ('wgrad', (32, 16, 16, 576), 384, (32, 16, 16, 576), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 16, 16, 576), 576, (32, 16, 16, 576), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 16, 16, 768), 0, (32, 16, 16, 768), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 16, 16, 768), 576, (32, 16, 16, 576), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 16, 16, 960), 0, (32, 16, 16, 576), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 32, 32, 128), 0, (32, 32, 32, 128), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 32, 32, 128), 0, (32, 32, 32, 256), 1, 0, 1, 0, False, False),
        ('wgrad', (32, 32, 32, 128), 0, (32, 32, 32, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 32, 32, 192), 0, (32, 32, 32, 192), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 32, 32, 192), 0, (32, 32, 32, 384), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 32, 32, 192), 0, (32, 32, 32, 384), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 32, 32, 256), 0, (32, 32, 32, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 32, 32, 384), 0, (32, 32, 32, 1152), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 32, 32, 384), 0, (32, 32, 32, 384), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 32, 32, 384), 0, (32, 32, 32, 384), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 32, 32, 384), 0, (32, 64, 64, 384), 3, 1, 1, 1, False, True),
        ('wgrad', (32, 32, 32, 384), 192, (32, 32, 32, 384), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 32, 32, 384), 384, (32, 32, 32, 384), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 32, 32, 576), 0, (32, 32, 32, 384), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 32, 32, 576), 0, (32, 32, 32, 576), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 32, 32, 576), 384, (32, 32, 32, 384), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 32, 32, 768), 0, (32, 32, 32, 384), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 32, 32, 960), 0, (32, 32, 32, 384), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 64, 64, 128), 0, (32, 64, 64, 128), 1, 0, 1, 0, False, False),
        ('wgrad', (32, 64, 64, 128), 0, (32, 64, 64, 128), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 64, 64, 192), 0, (32, 64, 64, 192), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 64, 64, 192), 0, (32, 64, 64, 64), 3, 1, 1, 0, False, False),
        ('wgrad', (32, 64, 64, 192), 192, (32, 64, 64, 192), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 64, 64, 384), 0, (32, 64, 64, 192), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 64, 64, 384), 0, (32, 64, 64, 384), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 64, 64, 384), 192, (32, 64, 64, 192), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 64, 64, 576), 0, (32, 64, 64, 192), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 64, 64, 64), 0, (32, 64, 64, 128), 1, 0, 1, 0, False, False),
        ('wgrad', (32, 64, 64, 64), 0, (32, 64, 64, 192), 1, 0, 1, 0, False, False),
        ('wgrad', (32, 8, 8, 1344), 0, (32, 8, 8, 768), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 8, 8, 1536), 0, (32, 8, 8, 768), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 8, 8, 256), 0, (32, 8, 8, 256), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 8, 8, 576), 0, (32, 8, 8, 576), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 8, 8, 576), 0, (32, 8, 8, 768), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 8, 8, 576), 0, (32, 8, 8, 768), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 8, 8, 768), 0, (32, 16, 16, 768), 3, 1, 1, 1, False, True),
        ('wgrad', (32, 8, 8, 768), 0, (32, 8, 8, 2304), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 8, 8, 768), 0, (32, 8, 8, 768), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 8, 8, 768), 0, (32, 8, 8, 768), 3, 1, 1, 0, False, True),
        ('wgrad', (32, 8, 8, 768), 576, (32, 8, 8, 768), 1, 0, 1, 0, False, True),
        ('wgrad', (32, 8, 8, 768), 768, (32, 8, 8, 768), 1, 0, 1, 0, False, True),
    ],
    'stem_wgrad': [
        # (op, x NCHW, dy NHWC)
        ('stem_wgrad', (128, 3, 32, 32), (128, 32, 32, 128)),
        ('stem_wgrad', (16, 3, 64, 64), (16, 64, 64, 128)),
        ('stem_wgrad', (16, 3, 64, 64), (16, 64, 64, 192)),
        ('stem_wgrad', (256, 3, 32, 32), (256, 32, 32, 128)),
        ('stem_wgrad', (32, 3, 64, 64), (32, 64, 64, 128)),
        ('stem_wgrad', (32, 3, 64, 64), (32, 64, 64, 192)),
    ],
    'linear_bwd': [
        # (op, x [P, K], dy [P, M], need_dx)
        ('linear_bwd', (128, 128), (128, 512), False),
        ('linear_bwd', (128, 512), (128, 4992), True),
        ('linear_bwd', (128, 512), (128, 512), True),
        ('linear_bwd', (16, 192), (16, 768), False),
        ('linear_bwd', (16, 768), (16, 35712), True),
        ('linear_bwd', (16, 768), (16, 768), True),
        ('linear_bwd', (32, 192), (32, 768), False),
        ('linear_bwd', (32, 768), (32, 35712), True),
        ('linear_bwd', (32, 768), (32, 768), True),
    ],
    'conv2d': [
        # (op, x NHWC, C1, Cout, k, transpose-flipped pack, stride, pad, pad_br, upsample, residual, mask_src, bias, act, out_nchw_f32)
        ('conv2d', (128, 16, 16, 128), 0, 128, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (128, 16, 16, 128), 0, 128, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (128, 16, 16, 128), 0, 128, 3, True, 1, 2, 0, 2, False, False, False, 0, False),
        ('conv2d', (128, 16, 16, 256), 0, 128, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 16, 16, 256), 0, 128, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (128, 16, 16, 256), 0, 128, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 16, 16, 256), 0, 128, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (128, 16, 16, 256), 0, 256, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 16, 16, 256), 0, 256, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (128, 16, 16, 256), 0, 256, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 16, 16, 256), 0, 256, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (128, 16, 16, 256), 0, 384, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 16, 16, 256), 0, 512, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 16, 16, 768), 0, 256, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 32, 32, 128), 0, 128, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 32, 32, 128), 0, 128, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (128, 32, 32, 128), 0, 128, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 32, 32, 128), 0, 128, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (128, 32, 32, 128), 0, 128, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (128, 32, 32, 128), 0, 256, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (128, 32, 32, 128), 0, 256, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 32, 32, 128), 0, 3, 3, True, 1, 1, None, 0, False, False, False, 0, True),
        ('conv2d', (128, 32, 32, 128), 0, 384, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 32, 32, 256), 0, 256, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 32, 32, 64), 0, 128, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 4, 4, 256), 0, 256, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 4, 4, 256), 0, 256, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (128, 4, 4, 256), 0, 256, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 4, 4, 256), 0, 256, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (128, 4, 4, 256), 0, 256, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (128, 4, 4, 256), 0, 256, 3, True, 1, 2, 0, 2, False, False, False, 0, False),
        ('conv2d', (128, 4, 4, 256), 0, 512, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 4, 4, 768), 0, 256, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 8, 8, 256), 0, 256, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 8, 8, 256), 0, 256, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (128, 8, 8, 256), 0, 256, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (128, 8, 8, 256), 0, 256, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (128, 8, 8, 256), 0, 256, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (128, 8, 8, 256), 0, 256, 3, True, 1, 2, 0, 2, False, False, False, 0, False),
        ('conv2d', (128, 8, 8, 256), 0, 512, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 16, 16, 1728), 0, 576, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 16, 16, 256), 0, 256, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 16, 16, 256), 0, 256, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (16, 16, 16, 256), 0, 256, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (16, 16, 16, 384), 0, 384, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 16, 16, 576), 0, 1152, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 16, 16, 576), 0, 1344, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 16, 16, 576), 0, 384, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (16, 16, 16, 576), 0, 384, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 16, 16, 576), 0, 576, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 16, 16, 576), 0, 576, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (16, 16, 16, 576), 0, 576, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 16, 16, 576), 0, 768, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (16, 16, 16, 576), 0, 960, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 16, 16, 768), 0, 768, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 32, 32, 1152), 0, 384, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 32, 32, 128), 0, 128, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (16, 32, 32, 128), 0, 128, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (16, 32, 32, 192), 0, 192, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 32, 32, 256), 0, 128, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 32, 32, 256), 0, 128, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (16, 32, 32, 256), 0, 256, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (16, 32, 32, 384), 0, 192, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (16, 32, 32, 384), 0, 192, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 32, 32, 384), 0, 384, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 32, 32, 384), 0, 384, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (16, 32, 32, 384), 0, 384, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 32, 32, 384), 0, 576, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (16, 32, 32, 384), 0, 576, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 32, 32, 384), 0, 768, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 32, 32, 384), 0, 960, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 32, 32, 576), 0, 576, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 64, 64, 128), 0, 128, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 64, 64, 128), 0, 128, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (16, 64, 64, 128), 0, 128, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (16, 64, 64, 128), 0, 3, 3, True, 1, 1, None, 0, False, False, False, 0, True),
        ('conv2d', (16, 64, 64, 192), 0, 192, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (16, 64, 64, 192), 0, 192, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 64, 64, 192), 0, 384, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (16, 64, 64, 192), 0, 384, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 64, 64, 192), 0, 576, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 64, 64, 384), 0, 384, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 64, 64, 64), 0, 192, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 8, 8, 2304), 0, 768, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 8, 8, 256), 0, 256, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (16, 8, 8, 256), 0, 256, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (16, 8, 8, 576), 0, 576, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 8, 8, 768), 0, 1344, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 8, 8, 768), 0, 1536, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 8, 8, 768), 0, 576, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (16, 8, 8, 768), 0, 576, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 8, 8, 768), 0, 768, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (16, 8, 8, 768), 0, 768, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (16, 8, 8, 768), 0, 768, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (256, 16, 16, 128), 0, 128, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (256, 16, 16, 128), 0, 128, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (256, 16, 16, 256), 0, 128, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (256, 16, 16, 256), 0, 128, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (256, 16, 16, 256), 0, 256, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (256, 32, 32, 128), 0, 128, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (256, 32, 32, 128), 0, 128, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (256, 32, 32, 128), 0, 128, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (256, 4, 4, 256), 0, 256, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (256, 4, 4, 256), 0, 256, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (256, 8, 8, 256), 0, 256, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (256, 8, 8, 256), 0, 256, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (256, 8, 8, 256), 0, 256, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (32, 16, 16, 1728), 0, 576, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 16, 16, 256), 0, 256, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 16, 16, 256), 0, 256, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (32, 16, 16, 256), 0, 256, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (32, 16, 16, 384), 0, 384, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 16, 16, 576), 0, 1152, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 16, 16, 576), 0, 1344, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 16, 16, 576), 0, 384, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (32, 16, 16, 576), 0, 384, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 16, 16, 576), 0, 576, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 16, 16, 576), 0, 576, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (32, 16, 16, 576), 0, 576, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 16, 16, 576), 0, 768, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (32, 16, 16, 576), 0, 960, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 16, 16, 768), 0, 768, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 32, 32, 1152), 0, 384, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 32, 32, 128), 0, 128, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (32, 32, 32, 128), 0, 128, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (32, 32, 32, 192), 0, 192, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 32, 32, 256), 0, 128, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 32, 32, 256), 0, 128, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (32, 32, 32, 256), 0, 256, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (32, 32, 32, 384), 0, 192, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (32, 32, 32, 384), 0, 192, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 32, 32, 384), 0, 384, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 32, 32, 384), 0, 384, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (32, 32, 32, 384), 0, 384, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 32, 32, 384), 0, 576, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (32, 32, 32, 384), 0, 576, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 32, 32, 384), 0, 768, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 32, 32, 384), 0, 960, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 32, 32, 576), 0, 576, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 64, 64, 128), 0, 128, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 64, 64, 128), 0, 128, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (32, 64, 64, 128), 0, 128, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (32, 64, 64, 192), 0, 192, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (32, 64, 64, 192), 0, 192, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 64, 64, 192), 0, 384, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (32, 64, 64, 192), 0, 384, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 64, 64, 192), 0, 576, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 64, 64, 384), 0, 384, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 64, 64, 64), 0, 192, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 8, 8, 2304), 0, 768, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 8, 8, 256), 0, 256, 3, True, 1, 1, None, 0, False, True, False, 0, False),
        ('conv2d', (32, 8, 8, 256), 0, 256, 3, True, 1, 1, None, 0, True, False, False, 0, False),
        ('conv2d', (32, 8, 8, 576), 0, 576, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 8, 8, 768), 0, 1344, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 8, 8, 768), 0, 1536, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 8, 8, 768), 0, 576, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (32, 8, 8, 768), 0, 576, 3, True, 1, 1, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 8, 8, 768), 0, 768, 1, True, 1, 0, None, 0, False, False, False, 0, False),
        ('conv2d', (32, 8, 8, 768), 0, 768, 1, True, 1, 0, None, 0, True, False, False, 0, False),
        ('conv2d', (32, 8, 8, 768), 0, 768, 3, True, 1, 1, None, 0, False, False, False, 0, False),
    ],
    'groupnorm_generic_bwd': [
        # (op, x NHWC, C1, add0, add1, groups, silu, scale_shift, fwd_stats)
        ('groupnorm_generic_bwd', (128, 16, 16, 256), 128, False, False, 32, True, False, False),
        ('groupnorm_generic_bwd', (128, 32, 32, 256), 128, False, False, 32, True, False, False),
        ('groupnorm_generic_bwd', (16, 16, 16, 384), 0, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (16, 16, 16, 384), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (16, 16, 16, 576), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (16, 16, 16, 576), 0, True, False, 32, False, False, True),
        ('groupnorm_generic_bwd', (16, 16, 16, 576), 0, True, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (16, 16, 16, 576), 384, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (16, 16, 16, 576), 576, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (16, 16, 16, 768), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (16, 16, 16, 768), 576, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (16, 32, 32, 192), 0, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (16, 32, 32, 192), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (16, 32, 32, 384), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (16, 32, 32, 384), 0, True, False, 32, False, False, True),
        ('groupnorm_generic_bwd', (16, 32, 32, 384), 0, True, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (16, 32, 32, 384), 192, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (16, 32, 32, 384), 384, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (16, 32, 32, 576), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (16, 32, 32, 576), 384, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (16, 64, 64, 192), 0, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (16, 64, 64, 192), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (16, 64, 64, 192), 0, True, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (16, 64, 64, 192), 192, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (16, 64, 64, 384), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (16, 64, 64, 384), 192, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (16, 8, 8, 576), 0, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (16, 8, 8, 576), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (16, 8, 8, 768), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (16, 8, 8, 768), 0, True, False, 32, False, False, False),
        ('groupnorm_generic_bwd', (16, 8, 8, 768), 0, True, False, 32, True, False, False),
        ('groupnorm_generic_bwd', (16, 8, 8, 768), 576, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (16, 8, 8, 768), 768, False, False, 32, True, False, False),
        ('groupnorm_generic_bwd', (32, 16, 16, 384), 0, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (32, 16, 16, 384), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (32, 16, 16, 576), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (32, 16, 16, 576), 0, True, False, 32, False, False, True),
        ('groupnorm_generic_bwd', (32, 16, 16, 576), 0, True, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (32, 16, 16, 576), 384, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (32, 16, 16, 576), 576, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (32, 16, 16, 768), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (32, 16, 16, 768), 576, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (32, 32, 32, 192), 0, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (32, 32, 32, 192), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (32, 32, 32, 384), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (32, 32, 32, 384), 0, True, False, 32, False, False, True),
        ('groupnorm_generic_bwd', (32, 32, 32, 384), 0, True, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (32, 32, 32, 384), 192, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (32, 32, 32, 384), 384, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (32, 32, 32, 576), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (32, 32, 32, 576), 384, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (32, 64, 64, 192), 0, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (32, 64, 64, 192), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (32, 64, 64, 192), 0, True, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (32, 64, 64, 192), 192, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (32, 64, 64, 384), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (32, 64, 64, 384), 192, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (32, 8, 8, 576), 0, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (32, 8, 8, 576), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (32, 8, 8, 768), 0, False, False, 32, True, True, True),
        ('groupnorm_generic_bwd', (32, 8, 8, 768), 0, True, False, 32, False, False, False),
        ('groupnorm_generic_bwd', (32, 8, 8, 768), 0, True, False, 32, True, False, False),
        ('groupnorm_generic_bwd', (32, 8, 8, 768), 576, False, False, 32, True, False, True),
        ('groupnorm_generic_bwd', (32, 8, 8, 768), 768, False, False, 32, True, False, False),
    ],
    'groupnorm_silu_bwd': [
        # (op, x NHWC, C1, add0, add1, groups, silu, scale_shift, fwd_stats)
        ('groupnorm_silu_bwd', (128, 16, 16, 128), 0, False, False, 32, True, False, False),
        ('groupnorm_silu_bwd', (128, 16, 16, 256), 0, False, False, 32, True, False, False),
        ('groupnorm_silu_bwd', (128, 16, 16, 256), 0, True, False, 32, False, False, False),
        ('groupnorm_silu_bwd', (128, 16, 16, 256), 0, True, False, 32, True, False, False),
        ('groupnorm_silu_bwd', (128, 16, 16, 256), 128, False, False, 32, True, False, False),
        ('groupnorm_silu_bwd', (128, 16, 16, 256), 256, False, False, 32, True, False, False),
        ('groupnorm_silu_bwd', (128, 32, 32, 128), 0, False, False, 32, True, False, False),
        ('groupnorm_silu_bwd', (128, 32, 32, 128), 0, True, False, 32, True, False, False),
        ('groupnorm_silu_bwd', (128, 32, 32, 128), 128, False, False, 32, True, False, False),
        ('groupnorm_silu_bwd', (128, 32, 32, 256), 128, False, False, 32, True, False, False),
        ('groupnorm_silu_bwd', (128, 4, 4, 256), 0, False, False, 32, True, False, False),
        ('groupnorm_silu_bwd', (128, 4, 4, 256), 0, True, False, 32, False, False, False),
        ('groupnorm_silu_bwd', (128, 4, 4, 256), 0, True, False, 32, True, False, False),
        ('groupnorm_silu_bwd', (128, 4, 4, 256), 256, False, False, 32, True, False, False),
        ('groupnorm_silu_bwd', (128, 8, 8, 256), 0, False, False, 32, True, False, False),
        ('groupnorm_silu_bwd', (128, 8, 8, 256), 0, True, False, 32, True, False, False),
        ('groupnorm_silu_bwd', (128, 8, 8, 256), 256, False, False, 32, True, False, False),
    ],
    'attention_bwd': [
        # (op, qkv [N, T, 3C], heads, o, lse)
        ('attention_bwd', (128, 16, 768), 1, False, False),
        ('attention_bwd', (128, 256, 768), 1, False, False),
        ('attention_bwd', (16, 1024, 1152), 6, True, True),
        ('attention_bwd', (16, 256, 1728), 9, True, True),
        ('attention_bwd', (16, 64, 2304), 12, True, True),
        ('attention_bwd', (32, 1024, 1152), 6, True, True),
        ('attention_bwd', (32, 256, 1728), 9, True, True),
        ('attention_bwd', (32, 64, 2304), 12, True, True),
    ],
    'colsum': [
        # (op, x, accumulate)
        ('colsum', (128, 32, 32, 128), False),
        ('colsum', (16, 64, 64, 128), False),
        ('colsum', (16, 64, 64, 192), False),
        ('colsum', (256, 32, 32, 128), False),
        ('colsum', (32, 64, 64, 128), False),
        ('colsum', (32, 64, 64, 192), False),
    ],
    'colsum_per_image': [
        # (op, x NHWC)
        ('colsum_per_image', (128, 16, 16, 256)),
        ('colsum_per_image', (128, 32, 32, 128)),
        ('colsum_per_image', (128, 4, 4, 256)),
        ('colsum_per_image', (128, 8, 8, 256)),
    ],
    'pool_act_bwd': [
        # (op, dout NHWC, pool)
        ('pool_act_bwd', (128, 16, 16, 128), False),
        ('pool_act_bwd', (128, 16, 16, 128), True),
        ('pool_act_bwd', (128, 32, 32, 128), False),
        ('pool_act_bwd', (128, 4, 4, 256), False),
        ('pool_act_bwd', (128, 4, 4, 256), True),
        ('pool_act_bwd', (128, 8, 8, 256), False),
        ('pool_act_bwd', (128, 8, 8, 256), True),
        ('pool_act_bwd', (16, 16, 16, 256), False),
        ('pool_act_bwd', (16, 16, 16, 256), True),
        ('pool_act_bwd', (16, 32, 32, 128), False),
        ('pool_act_bwd', (16, 32, 32, 128), True),
        ('pool_act_bwd', (16, 64, 64, 128), False),
        ('pool_act_bwd', (16, 8, 8, 256), False),
        ('pool_act_bwd', (16, 8, 8, 256), True),
        ('pool_act_bwd', (256, 16, 16, 128), False),
        ('pool_act_bwd', (256, 16, 16, 128), True),
        ('pool_act_bwd', (256, 32, 32, 128), False),
        ('pool_act_bwd', (256, 4, 4, 256), False),
        ('pool_act_bwd', (256, 4, 4, 256), True),
        ('pool_act_bwd', (256, 8, 8, 256), False),
        ('pool_act_bwd', (256, 8, 8, 256), True),
        ('pool_act_bwd', (32, 16, 16, 256), False),
        ('pool_act_bwd', (32, 16, 16, 256), True),
        ('pool_act_bwd', (32, 32, 32, 128), False),
        ('pool_act_bwd', (32, 32, 32, 128), True),
        ('pool_act_bwd', (32, 64, 64, 128), False),
        ('pool_act_bwd', (32, 8, 8, 256), False),
        ('pool_act_bwd', (32, 8, 8, 256), True),
    ],
    'upsample2x': [
        # (op, x NHWC)
        ('upsample2x', (16, 16, 16, 384)),
        ('upsample2x', (16, 32, 32, 192)),
        ('upsample2x', (16, 8, 8, 576)),
        ('upsample2x', (32, 16, 16, 384)),
        ('upsample2x', (32, 32, 32, 192)),
        ('upsample2x', (32, 8, 8, 576)),
    ],
    'dropout': [
        # (op, x NHWC, p, seed on the device)
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
        ('dropout', (32, 16, 16, 384), 0.1, False),
        ('dropout', (32, 16, 16, 576), 0.1, False),
        ('dropout', (32, 16, 16, 768), 0.1, False),
        ('dropout', (32, 32, 32, 192), 0.1, False),
        ('dropout', (32, 32, 32, 384), 0.1, False),
        ('dropout', (32, 32, 32, 576), 0.1, False),
        ('dropout', (32, 64, 64, 192), 0.1, False),
        ('dropout', (32, 64, 64, 384), 0.1, False),
        ('dropout', (32, 8, 8, 576), 0.1, False),
        ('dropout', (32, 8, 8, 768), 0.1, False),
    ],
    'value_head_bwd': [
        # (op, feat NHWC)
        ('value_head_bwd', (128, 4, 4, 256)),
        ('value_head_bwd', (16, 8, 8, 256)),
        ('value_head_bwd', (256, 4, 4, 256)),
        ('value_head_bwd', (32, 8, 8, 256)),
    ],
    'edm_dsm_loss_bwd': [
        # (op, x_start, weight schedule, distillation, g_mse, g_xs)
        ('edm_dsm_loss_bwd', (16, 3, 64, 64), 'karras', False, True, False),
        ('edm_dsm_loss_bwd', (32, 3, 64, 64), 'karras', False, True, False),
    ],
    'silu_bwd': [
        # (op, pre shape, pre dtype, g dtype)
        ('silu_bwd', (128, 512), 'float32', 'float32'),
        ('silu_bwd', (16, 768), 'float32', 'float32'),
        ('silu_bwd', (32, 768), 'float32', 'float32'),
    ],
    'var_step_bwd': [
        # (op, z, g_next, g_mean, g_control, g_logp)
        ('var_step_bwd', (128, 3, 32, 32), True, True, True, True),
    ],
    'linear': [
        # (op, P, K, Cout, pre_act, post_act, bias, form, split-K slices): forward kernels launched by the backward() methods
        ('linear', 128, 128, 512, 0, 0, True, 'small', 1),
        ('linear', 128, 4992, 512, 0, 0, False, 'small', 9),
        ('linear', 128, 512, 512, 0, 0, False, 'small', 1),
        ('linear', 128, 512, 512, 0, 0, True, 'small', 1),
        ('linear', 16, 192, 768, 0, 0, True, 'small', 1),
        ('linear', 16, 35712, 768, 0, 0, False, 'small', 64),
        ('linear', 16, 768, 768, 0, 0, False, 'small', 1),
        ('linear', 16, 768, 768, 0, 0, True, 'small', 1),
        ('linear', 32, 192, 768, 0, 0, True, 'small', 1),
        ('linear', 32, 35712, 768, 0, 0, False, 'small', 64),
        ('linear', 32, 768, 768, 0, 0, False, 'small', 1),
        ('linear', 32, 768, 768, 0, 0, True, 'small', 1),
    ],
    'pool_act': [
        # (op, x NHWC, pool, act)
        ('pool_act', (128, 16, 16, 256), True, 0),
        ('pool_act', (128, 32, 32, 256), True, 0),
        ('pool_act', (128, 8, 8, 256), True, 0),
        ('pool_act', (16, 16, 16, 768), True, 0),
        ('pool_act', (16, 32, 32, 576), True, 0),
        ('pool_act', (16, 64, 64, 384), True, 0),
        ('pool_act', (32, 16, 16, 768), True, 0),
        ('pool_act', (32, 32, 32, 576), True, 0),
        ('pool_act', (32, 64, 64, 384), True, 0),
    ],
    'value_head_pgrad': [
        # (op, s [N, C], learn_out_scale)
        ('value_head_pgrad', (128, 256), True),
        ('value_head_pgrad', (16, 256), True),
        ('value_head_pgrad', (256, 256), True),
        ('value_head_pgrad', (32, 256), True),
    ],
    'td_loss': [
        # (op, B, extra)
        ('td_loss', 128, True),
    ],
    'edm_step_bwd': [
        # (op, z, g_sample, g_mean)
        ('edm_step_bwd', (16, 3, 64, 64), True, True),
    ],
}

# 1x1 / 3x3 weight-gradient shapes outside the training steps that reach the register-staged families the census does not
# (4x4-wide maps, stride-2 1x1): every family the plan query can return is launched by some case
EXTRA_WGRAD = [
    ("wgrad", (8, 4, 4, 192), 0, (8, 4, 4, 128), 1, 0, 1, 0, False, True),          # conv_wgrad_kernel<1, true>
    ("wgrad", (4, 64, 64, 192), 0, (4, 32, 32, 128), 1, 0, 2, 0, False, True),      # conv_wgrad_kernel<1, false>
    ("wgrad", (6, 8, 4, 128), 64, (6, 8, 4, 128), 3, 1, 1, 0, False, True),          # conv_wgrad_kernel<3, true>
]
ALL_FAMILIES = {"b128_1x1", "ws3", "ws1", "reg3_pf", "reg3", "reg1_pf", "reg1"}


def _plan(ops, r):
    _, xs, c1, dys, k, pad, stride, ups, _, _ = r
    N, IH, IW, C0 = xs
    _, OH, OW, Co = dys
    return ops.conv2d_wgrad_plan(N, IH, IW, OH, OW, C0, c1, Co, k, stride, pad, ups)


def _id(r):
    return "-".join(str(v).replace(" ", "") for v in r[1:])


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    return o


def bf(t):
    return t.to(torch.bfloat16)


def rnd(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, device=DEV) * scale


def test_table_reaches_every_wgrad_family(ops):
    """The cases launch every family dxmi_conv2d_wgrad_plan can return; the training steps themselves reach these four."""
    fam_train = {_plan(ops, r)["family"] for r in CASES["wgrad"]}
    assert {"b128_1x1", "ws1", "ws3", "reg3"} <= fam_train
    fam_all = fam_train | {_plan(ops, r)["family"] for r in EXTRA_WGRAD}
    assert fam_all == ALL_FAMILIES, fam_all


import backward_census  # noqa: E402

# op kinds every recording must contain (a silently empty recording fails), and the kinds of each program beyond those
MIN_KINDS = {"wgrad", "conv2d", "stem_wgrad", "linear_bwd", "colsum", "silu_bwd", "dropout", "linear", "pool_act"}
PROGRAM_KINDS = {
    "imagenet64": {"attention_bwd", "groupnorm_generic_bwd", "pool_act_bwd", "value_head_bwd", "value_head_pgrad", "edm_step_bwd",
                   "upsample2x"},
    "cifar10": {"attention_bwd", "groupnorm_silu_bwd", "pool_act_bwd", "value_head_bwd", "value_head_pgrad", "var_step_bwd", "td_loss"},
    "edm_dsm_b16": {"attention_bwd", "groupnorm_generic_bwd", "edm_dsm_loss_bwd", "upsample2x"},
    "edm_dsm_b32": {"attention_bwd", "groupnorm_generic_bwd", "edm_dsm_loss_bwd", "upsample2x"},
}


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(backward_census.PROGRAMS))
def test_census_is_covered(ops, which):
    ops.device_check()
    rows, unknown = backward_census.record(ops, which)
    assert not unknown, f"{which}: ops functions called inside a backward that are neither launch ops nor allowed: {unknown}"
    table = {r for v in CASES.values() for r in v if not isinstance(r, str)}
    missing = sorted(rows - table, key=repr)
    assert not missing, f"{which}: backward launches not in CASES (add them): {missing}"
    need = (MIN_KINDS - ({"dropout"} if which == "imagenet64" else set())) | PROGRAM_KINDS[which]      # imagenet64_T10 has dropout 0
    assert {r[0] for r in rows} >= need, need - {r[0] for r in rows}
    torch.cuda.empty_cache()


def test_census_lists_are_consistent(ops):
    """Host-side: the launch ops, the allow-list and the class list of the censuses name only things `ops` has, and an op is
    recorded or allowed, not both.  (Functions on none of the lists are refused at run time, when a program calls them.)"""
    import forward_census
    fns = set(backward_census.public_functions(ops))
    launch, allowed = set(backward_census.OPS), set(backward_census.ALLOWED)
    fwd = set(forward_census.FWD_OPS + forward_census.STEP_OPS)
    assert launch <= fns and allowed <= fns and fwd <= fns, sorted((launch | allowed | fwd) - fns)
    assert not (launch & allowed) and not (fwd & allowed)
    assert not backward_census.unknown_classes(ops)
    assert set(backward_census._NEW) <= launch


def test_every_row_kind_has_a_test():
    """Host-side: the op kinds of CASES are exactly the kinds some test of this file parametrises over."""
    import re
    src = open(__file__).read()
    tested = set(re.findall(r'CASES\["([a-z0-9_]+)"\]', src))
    assert set(CASES) == tested, set(CASES) ^ tested


# ------------------------------------------------------------------------------------------ weight gradients
@pytest.mark.gpu
@pytest.mark.parametrize("r", CASES["wgrad"] + EXTRA_WGRAD, ids=_id)
def test_wgrad(ops, r):
    """dW (and db) of dxmi_conv2d_wgrad[_bias] element by element within c * u32 * sum|dy||x|, c from the plan's chain
    length; accumulate=True must give bitwise twice the first result."""
    _, xs, c1, dys, k, pad, stride, ups, _, with_bias = r
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(r).encode()))
    x0 = bf(rnd(g, *xs))
    x1 = bf(rnd(g, *xs[:3], c1, scale=2.0)) if c1 else None
    dy = bf(rnd(g, *dys))
    plan = _plan(ops, r)
    wgrad_checked(ops, x0, dy, k, CHECK, in1=x1, pad=pad, stride=stride, upsample=bool(ups), with_bias=with_bias,
                  tag=f"wgrad[{plan['family']}]")


@pytest.mark.gpu
@pytest.mark.parametrize("r", CASES["stem_wgrad"], ids=_id)
def test_stem_conv_wgrad(ops, r):
    _, xs, dys = r
    g = torch.Generator(device=DEV).manual_seed(7)
    x = rnd(g, *xs)
    dy = bf(rnd(g, *dys))
    N, _, H, W = xs
    got = ops.stem_conv_wgrad(x, dy)
    xb = bf(x).permute(0, 2, 3, 1)                              # the im2col operand is the bf16-rounded image
    ref, A = wgrad_ref(xb, dy, 3)
    plan = ops.conv2d_wgrad_plan(N, H, W, H, W, 64, 0, dys[3], 1)
    CHECK.fp32("stem_wgrad", got, ref, A, wgrad_depth(plan))


@pytest.mark.gpu
@pytest.mark.parametrize("r", CASES["linear_bwd"], ids=_id)
def test_linear_bwd(ops, r):
    """linear_bwd at the emb_layers / temb MLP sizes: dW through the 1x1 weight gradient on zero-padded rows, dx through the
    transposed-pack linear (bf16 operands, fp32 out), db."""
    _, xs, dys, need_dx = r
    P, K = xs
    M = dys[1]
    g = torch.Generator(device=DEV).manual_seed(11)
    x = rnd(g, P, K)
    dy = rnd(g, P, M, scale=0.1)
    W = rnd(g, M, K, scale=K ** -0.5)
    pw_t = ops.pack_conv_weight(W, transpose_flip=True) if need_dx else None
    dx, dw, db = ops.linear_bwd(x, dy, pw_t, need_dx=need_dx)
    xb, dyb = bf(x).double(), bf(dy).double()
    rows = 64
    while rows < P:
        rows *= 2
    plan = ops.conv2d_wgrad_plan(1, rows // 16, 16, rows // 16, 16, K, 0, M, 1)
    CHECK.fp32("linear_bwd_dw", dw, dyb.T @ xb, dyb.abs().T @ xb.abs(), wgrad_depth(plan))
    # db is dy.sum(0), a stock torch reduction inside linear_bwd (no project kernel): checked, not reported as kernel coverage
    Checker().fp32("linear_bwd_db", db, dy.double().sum(0), dy.double().abs().sum(0), P + 2)
    if need_dx:
        Wb = bf(W).double()
        CHECK.fp32("linear_bwd_dx", dx, dyb @ Wb, dyb.abs() @ Wb.abs(), 2 * M + 2)


@pytest.mark.gpu
@pytest.mark.parametrize("r", CASES["colsum"] + CASES["colsum_per_image"], ids=_id)
def test_colsums(ops, r):
    g = torch.Generator(device=DEV).manual_seed(13)
    x = bf(rnd(g, *r[1]))
    N, H, W, C = x.shape
    xd = x.double()
    if r[0] == "colsum":
        got = ops.colsum(x)
        CHECK.fp32("colsum", got, xd.reshape(-1, C).sum(0), xd.abs().reshape(-1, C).sum(0), N * H * W + 2)
    else:
        got = ops.colsum_per_image(x)
        CHECK.fp32("colsum_per_image", got, xd.sum((1, 2)), xd.abs().sum((1, 2)), H * W + 2)


@pytest.mark.gpu
@pytest.mark.parametrize("r", CASES["pool_act_bwd"], ids=_id)
def test_pool_act_bwd(ops, r):
    """Value-net pool / LeakyReLU backward: din = (pool ? 0.25 * nearest-x2(g) : g), g = dout * (act_out > 0 ? 1 : 0.2), element
    by element: one fp32 product, one bf16 rounding."""
    _, ds, pool = r
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(r).encode()))
    dout = bf(rnd(g, *ds))
    act = bf(rnd(g, *ds))
    got = ops.pool_act_bwd(dout, act, pool, 0.2)
    ref = dout.double() * torch.where(act > 0, 1.0, 0.2).double()
    if pool:
        ref = 0.25 * ref.repeat_interleave(2, 1).repeat_interleave(2, 2)
    CHECK.bf16("pool_act_bwd", got, ref, ref.abs(), 2)


# ------------------------------------------------------------------------------------------ data gradients
def conv_ref(x, Wt, stride, pad, pad_br, ups, residual, mask, slope):
    """fp64 conv of the data-gradient launch: x NHWC, Wt [Cout, Cin, k, k] (the transpose-flipped forward weight)."""
    k = Wt.shape[2]
    xd = x.double()
    if ups == 1:
        xd = xd.repeat_interleave(2, 1).repeat_interleave(2, 2)
    elif ups == 2:
        z = torch.zeros(xd.shape[0], 2 * xd.shape[1], 2 * xd.shape[2], xd.shape[3], dtype=xd.dtype, device=xd.device)
        z[:, ::2, ::2] = xd
        xd = z
    N, VH, VW, _ = xd.shape
    pb = pad if pad_br is None else pad_br
    OH, OW = (VH + pad + pb - k) // stride + 1, (VW + pad + pb - k) // stride + 1
    cols = unfold_nhwc(xd, k, stride, pad, pb)                    # [N, Cin*k*k, OH*OW]
    Wm = Wt.double().reshape(Wt.shape[0], -1)
    out = torch.einsum("ok,nkp->npo", Wm, cols).reshape(N, OH, OW, -1)
    A = torch.einsum("ok,nkp->npo", Wm.abs(), cols.abs()).reshape(N, OH, OW, -1)
    if residual is not None:
        out, A = out + residual.double(), A + residual.double().abs()
    if mask is not None:
        f = torch.where(mask > 0, 1.0, slope).double()
        out, A = out * f, A * f
    return out, A


@pytest.mark.gpu
@pytest.mark.parametrize("tuning", ["default", "throughput"])
@pytest.mark.parametrize("r", CASES["conv2d"], ids=_id)
def test_conv_dgrad(ops, r, tuning):
    """The data-gradient convs (transpose-flipped packs, residual / activation-mask epilogues, zero-stuffed stride-2 transposes)
    element by element: c = Cin * k * k + 2, one bf16 rounding of the output.  The pack is made the way the census saw it
    (transpose-flipped or plain)."""
    _, xs, c1, Cout, k, tflip, stride, pad, pad_br, ups, has_res, has_mask, has_bias, act, nchw = r
    assert c1 == 0 and not has_bias and act == 0
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(r).encode()))
    x = bf(rnd(g, *xs))
    Cin = xs[3]
    if tflip:
        Wf = rnd(g, Cin, Cout, k, k, scale=(Cin * k * k) ** -0.5)  # the forward layer's weight [Cin_dg, Cout_dg, k, k]
        Wt = bf(Wf).float().transpose(0, 1).flip(2, 3)           # its transpose-flip: the weight of this launch
    else:
        Wf = rnd(g, Cout, Cin, k, k, scale=(Cin * k * k) ** -0.5)
        Wt = bf(Wf).float()
    pw = ops.pack_conv_weight(Wf, transpose_flip=tflip)
    assert pw.transpose_flip == tflip
    N, IH, IW, _ = xs
    VH, VW = (2 * IH, 2 * IW) if ups else (IH, IW)
    pb = pad if pad_br is None else pad_br
    OH, OW = (VH + pad + pb - k) // stride + 1, (VW + pad + pb - k) // stride + 1
    res = bf(rnd(g, N, OH, OW, Cout)) if has_res else None
    mask = bf(rnd(g, N, OH, OW, Cout)) if has_mask else None
    kw = dict(stride=stride, pad=pad, pad_br=pad_br, upsample=ups, residual=res, mask_src=mask, mask_slope=0.2, out_nchw_f32=nchw)
    if tuning == "throughput":
        with ops.throughput_tuning():
            got = ops.conv2d(x, pw, **kw)
    else:
        got = ops.conv2d(x, pw, **kw)
    ref, A = conv_ref(x, Wt, stride, pad, pad_br, ups, res, mask, 0.2)
    c = Cin * k * k + 2
    if nchw:
        CHECK.fp32("conv_dgrad_f32", got.permute(0, 2, 3, 1), ref, A, c)
    else:
        CHECK.bf16("conv_dgrad", got, ref, A, c)


# ------------------------------------------------------------------------------------------ GroupNorm
def _gn_case(ops, r, form):
    op, xs, c1, has_add0, has_add1, groups, silu, has_ss, has_saved = r
    N, H, W, C0 = xs
    C = C0 + c1
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(r).encode()))
    x0 = bf(rnd(g, *xs) * 1.5 + 0.25)
    x1 = bf(rnd(g, N, H, W, c1)) if c1 else None
    dy = bf(rnd(g, N, H, W, C))
    gamma, beta = 1 + 0.3 * rnd(g, C), 0.3 * rnd(g, C)
    add0 = bf(rnd(g, N, H, W, C0)) if has_add0 else None
    add1 = bf(rnd(g, N, H, W, c1)) if has_add1 else None
    ss = (0.3 * rnd(g, N, 3 * C))[:, C // 2: C // 2 + 2 * C] if has_ss else None     # a row-strided slice, as emb_all's
    eps = 1e-5 if op == "groupnorm_generic_bwd" else 1e-6
    saved = []
    if op == "groupnorm_generic_bwd" and has_saved:
        ops.groupnorm_generic(x0, gamma, beta, in1=x1, groups=groups, eps=eps, silu=silu, scale_shift=ss, saved=saved)
    gn_bwd_checked(ops, op, form, x0, dy, gamma, beta, CHECK, in1=x1, add0=add0, add1=add1, groups=groups, eps=eps, silu=silu,
                   scale_shift=ss, fwd_stats=saved[0] if saved else None)


@pytest.mark.gpu
@pytest.mark.parametrize("r", CASES["groupnorm_generic_bwd"] + CASES["groupnorm_silu_bwd"], ids=_id)
def test_groupnorm_bwd(ops, r):
    """dx (both concat sources, fused adds), dgamma, dbeta and the FiLM scale-shift gradient; the generic backward on every
    launch form its residency guard allows for the shape (knob gn_bwd_fused 0: two launches, 2: one launch where it fits)."""
    N, H, W, C0 = r[1]
    C = C0 + r[2]
    if r[0] == "groupnorm_silu_bwd":
        _gn_case(ops, r, "resident")
        return
    old = ops.get_tuning("gn_bwd_fused")
    try:
        forms = []
        for knob in (0, 2):
            ops.set_tuning("gn_bwd_fused", knob)
            f = ops.groupnorm_generic_bwd_plan(N, H * W, C)
            if f not in forms:
                forms.append(f)
                _gn_case(ops, r, "one-launch" if f else "two-launch")
        assert 0 in forms
    finally:
        ops.set_tuning("gn_bwd_fused", old)


# ------------------------------------------------------------------------------------------ attention
ATTN_EXTRA = [("attention_bwd", (16, 1024, 1152), 6, True, True), ("attention_bwd", (16, 256, 1728), 9, True, True),
              ("attention_bwd", (16, 64, 2304), 12, True, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("r", sorted(set(CASES["attention_bwd"]) | set(ATTN_EXTRA), key=repr), ids=_id)
def test_attention_bwd(ops, r):
    """dqkv per (image, q|k|v, head, 128-row block) within rel-L2 8 u16: P and dS are bf16 MFMA operands in the kernels, so the
    bound is per block at the kernel's tile size rather than per element.  With lse: the training path (o and the forward's
    log-sum-exp handed over)."""
    _, qs, heads, with_o, with_lse = r
    N, T, C3 = qs
    C = C3 // 3
    D = C // heads
    scale = D ** -0.5
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(r).encode()))
    qkv = bf(rnd(g, N, T, C3))
    do = bf(rnd(g, N, T, C))
    ref = attention_bwd_ref(qkv, do, heads, scale)
    o = lse = None
    if with_lse:
        o, lse = ops.attention(qkv, heads, scale, want_lse=True)
    elif with_o:
        o = bf(ref[1])
    attention_bwd_checked(ops, qkv, do, heads, scale, CHECK, o=o, lse=lse, ref=ref,
                          tag=f"attention_bwd[T{T},h{heads}{',lse' if with_lse else ''}]")


# ------------------------------------------------------------------------------------------ the ops outside the first ten
@pytest.mark.gpu
@pytest.mark.parametrize("r", CASES["silu_bwd"], ids=_id)
def test_silu_bwd(ops, r):
    """g * s (1 + x (1 - s)) in fp64 on the same fp32 inputs (pre-activations of the embedding MLP, a few units wide)."""
    _, shape, dt_pre, dt_g = r
    assert dt_pre == dt_g == "float32"
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(r).encode()))
    pre, gy = rnd(g, *shape, scale=3.0), rnd(g, *shape)
    got = ops.silu_bwd(pre, gy)
    assert got.dtype == torch.float32
    ref, A = silu_bwd_ref(pre, gy)
    CHECK.fp32("silu_bwd", got, ref, A, 16)


@pytest.mark.gpu
@pytest.mark.parametrize("r", CASES["dropout"], ids=_id)
def test_dropout_and_its_backward_replay(ops, r):
    """The kept set is bit-equal to the hash restatement, kept values are bf16(x / (1 - p)) of the fp64 quotient, the same seed
    on a second tensor (the gradient: the backward's replay, written in place as the nets do) keeps the same elements, and the
    next site of the step (dropout_site_seed(base, 1)) draws another mask."""
    _, shape, p, on_dev = r
    assert not on_dev
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(r).encode()))
    x, gy = bf(rnd(g, *shape)), bf(rnd(g, *shape))
    seed0, seed1 = ops.dropout_site_seed(1234, 0), ops.dropout_site_seed(1234, 1)
    y = ops.dropout(x, p, seed0)
    keep, ref, tie = dropout_ref(x, p, seed0)
    assert torch.equal((y != 0) | (x == 0), keep | (x == 0)), "kept set differs from the hash"
    bad = (y != ref) & ~tie
    assert not bool(bad.any()), f"{int(bad.sum())} kept values differ from bf16(x / (1 - p))"
    near = (y.double() - ref.double()).abs() <= 2 * U16 * ref.double().abs()
    assert bool(near.all())
    dgy = gy.clone()
    ops.dropout(dgy, p, seed0, out=dgy)
    _, gref, gtie = dropout_ref(gy, p, seed0)
    assert not bool(((dgy != gref) & ~gtie).any()), "the backward replay of the seed keeps other elements / values"
    y1 = ops.dropout(x, p, seed1)
    same = float(((y1 != 0) == (y != 0)).double().mean())
    assert seed0 != seed1 and same < 1 - p, f"two sites of one step share a mask (agreement {same})"
    CHECK._note("dropout[mismatches]", 0.0)


VALUE_HEAD_EXTRA = [("value_head_bwd", (64, 4, 4, 256)), ("value_head_bwd", (32, 4, 4, 256)), ("value_head_bwd", (512, 4, 4, 256))]


@pytest.mark.gpu
@pytest.mark.parametrize("r", CASES["value_head_bwd"] + VALUE_HEAD_EXTRA, ids=_id)
def test_value_head_bwd(ops, r):
    """dfeat = relu'(feat) w dy: one fp32 product, one bf16 store; s = sum_hw relu(feat): fp32 depth HW.  The census holds the
    pair batches of the recorded steps (2B and B); the extra rows are the pairs of the CIFAR-10 batches 256 and 32."""
    _, fs = r
    N, H, W, C = fs
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(r).encode()))
    feat = bf(rnd(g, *fs))
    w, dy = rnd(g, C, scale=C ** -0.5), rnd(g, N)
    dfeat, s = ops.value_head_bwd(feat, w, dy)
    rdf, rs, As = value_head_bwd_ref(feat, w, dy)
    CHECK.bf16("value_head_bwd_dfeat", dfeat, rdf, rdf.abs(), 2)
    CHECK.fp32("value_head_bwd_s", s, rs, As, H * W + 2)


PGRAD_EXTRA = [("value_head_pgrad", (n, 256), o) for n in (512, 256, 128, 64, 32) for o in (True, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("r", sorted(set(CASES["value_head_pgrad"]) | set(PGRAD_EXTRA), key=repr), ids=_id)
def test_value_head_pgrad(ops, r):
    """The four head-parameter gradients against fp64 autograd, with and without learn_out_scale, at the recorded batches and
    the pair batches of CIFAR-10 at 256 / 128 / 32."""
    _, (N, C), has_ow = r
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(r).encode()))
    s = rnd(g, N, C).abs() * 4
    w, b, dy = rnd(g, C, scale=C ** -0.5), rnd(g, 1), rnd(g, N)
    ow = rnd(g, 1, 1) if has_ow else None
    got = ops.value_head_pgrad(s, w, b, dy, ow)
    ref, A = value_head_pgrad_ref(s, w, b, dy, ow)
    CHECK.fp32("value_head_pgrad", got, ref, A, N + C + 8)


@pytest.mark.gpu
@pytest.mark.parametrize("r", CASES["td_loss"] + [("td_loss", 256, True), ("td_loss", 32, True), ("td_loss", 100, False)], ids=_id)
def test_td_loss(ops, r):
    from test_hip_forward_shapes import check_td_loss
    check_td_loss(ops, CHECK, r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", CASES["edm_dsm_loss_bwd"], ids=_id)
def test_edm_dsm_loss_bwd(ops, r):
    """d(model_out) of the DSM terms at the recorded batch: the fp64 expressions of
    test_hip_edm_dsm.py::test_dsm_kernels_vs_fp64 (operands, scalings64, weights64 imported), bound derived in
    backward_bounds.dsm_loss_bwd_ref."""
    from test_hip_edm_dsm import operands, scalings64, weights64
    _, shape, ws, distill, has_gm, has_gx = r
    N, CHW = shape[0], shape[1] * shape[2] * shape[3]
    x0, noise, F_, sig = [t.to(DEV) for t in operands(N, CHW, zlib.crc32(repr(r).encode()) % 1000)]
    g = torch.Generator(device=DEV).manual_seed(3)
    gm, gx = (rnd(g, N) if has_gm else None), (rnd(g, N) if has_gx else None)
    v4 = lambda t: t.view(shape).contiguous()
    dF = ops.edm_dsm_loss_bwd(gm, gx, v4(F_), v4(x0), v4(noise), sig, ws, distillation=distill)
    e, Me, c_out = dsm_error_terms(F_, x0, noise, sig, scalings64(sig, distill=distill))
    CHECK.fp32("edm_dsm_loss_bwd", dF.view(N, CHW), *dsm_loss_bwd_ref(e, Me, c_out, gm, gx, weights64(ws, sig)), 16)


@pytest.mark.gpu
@pytest.mark.parametrize("r", CASES["var_step_bwd"], ids=_id)
def test_var_step_bwd(ops, r):
    """dxmi_var_step_bwd at the recorded batch, per-sample scalars all different, against fp64 autograd
    (backward_bounds.var_step_bwd_ref)."""
    _, shape, *has = r
    N, CHW = shape[0], shape[1] * shape[2] * shape[3]
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(r).encode()))
    gs = [rnd(g, *shape) if h else None for h in has[:3]] + [rnd(g, N) if has[3] else None]
    z, cm, sg = rnd(g, *shape), -rnd(g, N).abs() - 0.1, torch.exp(rnd(g, N) * 0.3 - 1.0)
    d_eps, d_sigma = ops.var_step_bwd(*gs, z, cm, sg)
    f = lambda t: None if t is None else t.view(N, CHW)
    re_, rs, Ae, As = var_step_bwd_ref(f(gs[0]), f(gs[1]), f(gs[2]), gs[3], f(z), cm, sg)
    CHECK.fp32("var_step_bwd_deps", f(d_eps), re_, Ae, 8)
    CHECK.fp32("var_step_bwd_dsigma", d_sigma, rs, As, CHW + 8)


@pytest.mark.gpu
@pytest.mark.parametrize("r", CASES["edm_step_bwd"], ids=_id)
def test_edm_step_bwd(ops, r):
    """dxmi_edm_step_bwd at the recorded batch, one sigma per sample over the whole ladder, against fp64 autograd
    (backward_bounds.edm_step_bwd_ref)."""
    _, shape, has_gs, has_gm = r
    N, CHW = shape[0], shape[1] * shape[2] * shape[3]
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(r).encode()))
    gs, gm = (rnd(g, *shape) if has_gs else None), (rnd(g, *shape) if has_gm else None)
    z = rnd(g, *shape)
    sigma = torch.exp(torch.linspace(-6.2, 4.38, N, device=DEV))
    sdn = sigma * (0.2 + 0.6 * torch.rand(N, generator=g, device=DEV))
    d_out, d_up = ops.edm_step_bwd(gs, gm, z, sigma, sdn)
    f = lambda t: None if t is None else t.view(N, CHW)
    rF, rup, AF, Aup = edm_step_bwd_ref(f(gs), f(gm), f(z), sigma, sdn)
    CHECK.fp32("edm_step_bwd_dF", f(d_out), rF, AF, 16)
    CHECK.fp32("edm_step_bwd_dsigma_up", d_up, rup, Aup, CHW + 8)


@pytest.mark.gpu
@pytest.mark.parametrize("r", CASES["linear"], ids=_id)
def test_linear_in_backward(ops, r):
    """The forward `linear` launches of the backward() methods: recomputed pre-activations, and the transposed-pack dx of
    linear_bwd, which splits K (S slices: partial sums added in fp32, within the same depth-K bound)."""
    _, P, K, M, pre, post, has_bias, form, S = r
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(r).encode()))
    x = rnd(g, P, K)
    W = rnd(g, M, K, scale=K ** -0.5)
    bias = rnd(g, M, scale=0.1) if has_bias else None
    if S > 1:
        assert int(ops.load().dxmi_linear_splitk_slices(P, K, M)) == S
    got = ops.linear(x, ops.pack_conv_weight(W), bias, pre_act=pre, post_act=post, splitk=S > 1)
    ref, bound = linear_ref(x, W, bias, pre, post, depth=K + 2 + S if S > 1 else None)
    CHECK.within(f"linear[{form},S{'>1' if S > 1 else '=1'}]", got, ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("r", CASES["upsample2x"], ids=_id)
def test_upsample2x_in_backward(ops, r):
    x = bf(rnd(torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(r).encode())), *r[1]))
    assert torch.equal(ops.upsample2x(x), x.repeat_interleave(2, 1).repeat_interleave(2, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("r", CASES["pool_act"], ids=_id)
def test_pool_act_in_backward(ops, r):
    _, xs, pool, act = r
    x = bf(rnd(torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(r).encode())), *xs))
    CHECK.within("pool_act", ops.pool_act(x, pool, act), *pool_act_ref(x, pool, act))


@pytest.mark.gpu
def test_report():
    """Largest |err| / bound per op over the cases above (printed; run with -s)."""
    for k, v in CHECK.report().items():
        print(f"{k:48s} {v:.4f}")
