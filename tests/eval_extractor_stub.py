"""A weight-free stand-in for the evaluator's extractor (`--extractor eval_extractor_stub:PoolSpatialFeatures`), meeting the
contract documented on pytorch_fid.inception.EvalInceptionV3: uint8 NHWC images [B, H, W, 3] -> (pool [B, 64] f32,
spatial [B, 23] f32) on the images' device, plus a `softmax_weight` [64, 10].  Deterministic in the pixels; not a quality metric:
it exists so the evaluator's flow runs end to end without the Inception weight file."""
import torch

POOL, SPATIAL, CLASSES = 64, 23, 10


class PoolSpatialFeatures:
    def __init__(self):
        g = torch.Generator().manual_seed(5)
        w = torch.randn(POOL, CLASSES, generator=g) * 0.5
        self.softmax_weight = w.cuda() if torch.cuda.is_available() else w

    def __call__(self, images):
        x = images.float() / 255.0                                              # [B, H, W, 3]
        B = x.shape[0]
        q = torch.nn.functional.adaptive_avg_pool2d(x.permute(0, 3, 1, 2), 4).reshape(B, 48)      # channel x 4x4 cell means
        q2 = torch.nn.functional.adaptive_avg_pool2d(x[..., :1].permute(0, 3, 1, 2) ** 2, 4).reshape(B, 16)
        pool = torch.cat([q, q2], 1) * 4.0
        spatial = torch.nn.functional.adaptive_avg_pool2d(x.permute(0, 3, 1, 2), 3).reshape(B, 27)[:, :SPATIAL]
        return pool.contiguous(), spatial.contiguous()
