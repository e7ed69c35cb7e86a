"""CLI surface: `--a.b.c v` overrides, YAML/_target_ config layer, checkpoint key fix-up (CPU)."""
import os

import pytest
import torch


def test_parse_arg_type():
    from cmd_utils import parse_arg_type as p
    assert p("3") == 3 and isinstance(p("3"), int)
    assert p("1e-6") == 1e-6 and p("0.5") == 0.5 and p("-2") == -2.0
    assert p("true") is True and p("False") is False
    assert p("null") is None and p("None") is None
    assert p("[1,2,2,2]") == [1, 2, 2, 2]
    assert p("fix_last") == "fix_last"


def test_unknown_and_nested_args():
    from cmd_utils import parse_nested_args, parse_unknown_args
    d = parse_unknown_args(["--training.lr", "1e-6", "--trainer.tau1", "0.1", "--run", "x"])
    assert d == {"training.lr": 1e-6, "trainer.tau1": 0.1, "run": "x"}
    assert parse_nested_args(d) == {"training": {"lr": 1e-6}, "trainer": {"tau1": 0.1}, "run": "x"}
    with pytest.raises(AssertionError):
        parse_unknown_args(["--a=1", "2"])


def test_config_merge_instantiate_roundtrip(tmp_path):
    import configs_builtin
    import dxmi_config
    cfg = configs_builtin.get("cifar10_T10")
    cfg = dxmi_config.merge(cfg, {"training": {"lr": 1e-6}, "sampler": {"n_timesteps": 4}})
    assert cfg.training.lr == 1e-6 and cfg.training.v_lr == 1e-5 and cfg.sampler.n_timesteps == 4
    assert cfg.training.get("fid_every", None) is None and cfg.energy is None
    path = os.path.join(tmp_path, "config.yaml")
    dxmi_config.save(cfg, path)
    cfg2 = dxmi_config.load(path)
    assert dxmi_config.to_container(cfg2) == dxmi_config.to_container(cfg)
    net = dxmi_config.instantiate(cfg2.sampler_net)
    sampler = dxmi_config.instantiate(cfg2.sampler, net=net)
    assert type(sampler).__name__ == "VARSampler" and sampler.n_timesteps == 4 and sampler.net is net
    v = dxmi_config.instantiate(cfg2.value)
    assert type(v).__name__ == "TimeIndependentValue" and type(v.net).__name__ == "IGEBMEncoderV2"
    assert dxmi_config.instantiate(cfg2.energy) is None


def test_fix_legacy_dict():
    from utils import fix_legacy_dict
    sd = {"module.a.weight": torch.zeros(1), "module.b.bias": torch.ones(1)}
    out = fix_legacy_dict({"model": sd})
    assert list(out.keys()) == ["a.weight", "b.bias"]
    assert list(fix_legacy_dict({"state_dict": {"x": 1, "y": 2}}).keys()) == ["x", "y"]


def test_png_writer_roundtrip(tmp_path):
    """The thread-pool PNG writer produces standard 8-bit RGB PNGs with save_image's rounding."""
    import numpy as np
    import torch
    from PIL import Image
    from utils import to_uint8_nhwc, write_png_batch
    g = torch.Generator().manual_seed(0)
    x = torch.rand(9, 3, 32, 32, generator=g)
    u8 = to_uint8_nhwc(x)
    ref = x.mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).numpy()
    assert u8.shape == (9, 32, 32, 3) and np.array_equal(u8, ref)
    paths = [str(tmp_path / f"0_{i}.png") for i in range(9)]
    write_png_batch(u8, paths, workers=4)
    for i, p in enumerate(paths):
        im = Image.open(p)
        assert im.mode == "RGB" and im.size == (32, 32) and np.array_equal(np.asarray(im), u8[i])


# ---- YAML files through the loader and the scripts' config path ----------------------------------------------------------
def _write_config_files(tmp_path, name):
    """configs_builtin[name] as the two YAML files the training scripts read: --config without its data block, --dataset
    with it."""
    import configs_builtin
    import dxmi_config
    cfg = dxmi_config.to_container(configs_builtin.get(name))
    data = cfg.pop("data")
    model, dataset = str(tmp_path / f"{name}.yaml"), str(tmp_path / f"{name}_data.yaml")
    dxmi_config.save(cfg, model)
    dxmi_config.save({"data": data}, dataset)
    return model, dataset


def test_yaml_scalars_follow_omegaconf(tmp_path):
    """`1e-7` (no dot, unsigned exponent) is a string for PyYAML's YAML-1.1 resolver and a float for OmegaConf's loader
    (reference train_cifar10.py:228-233): the optimisers got lr='1e-7' (round-3 VERDICT).  Also Null / True / lists,
    timestamps stay strings, duplicate keys are an error."""
    import dxmi_config
    import yaml
    p = tmp_path / "c.yaml"
    p.write_text("a: 1e-7\nb: 1E5\nc: -2e+3\nd: 1.5e-3\ne: Null\nf: True\ng: 2001-01-01\nh: fix_last\ni: 10\n"
                 "j: [1,2,2,2]\nk: .5\nl: '1e-7'\nm: 1_000\nn: 0.0\no: 1.0e-06\np: 1e-8\n")
    c = dxmi_config.load(str(p))
    assert c.a == 1e-7 and isinstance(c.a, float) and c.b == 1e5 and isinstance(c.b, float) and c.c == -2000.0
    assert c.d == 1.5e-3 and c.e is None and c.f is True and c.g == "2001-01-01" and c.h == "fix_last"
    assert c.i == 10 and isinstance(c.i, int) and c.j == [1, 2, 2, 2] and c.k == 0.5 and c.l == "1e-7"
    assert c.m == 1000 and c.n == 0.0 and isinstance(c.n, float)
    assert c.o == 1e-6 and isinstance(c.o, float) and c.p == 1e-8 and isinstance(c.p, float)
    p.write_text("a: 1\na: 2\n")
    with pytest.raises(yaml.constructor.ConstructorError):
        dxmi_config.load(str(p))


def test_train_cifar10_config_to_optimizer_groups_dry_run(tmp_path):
    """No GPU: YAML files -> merged config -> net / sampler / value -> the Adam groups of train_cifar10.py:283-296."""
    import dxmi_config
    import train_cifar10
    cfg = train_cifar10.load_config(*_write_config_files(tmp_path, "cifar10_T10"),
                                    {"training": {"v_lr": 2e-5}})
    assert cfg.data.name == "cifar10" and cfg.training.batchsize == 128
    net = dxmi_config.instantiate(cfg.sampler_net)
    sampler = dxmi_config.instantiate(cfg.sampler, net=net)
    v = dxmi_config.instantiate(cfg.value)
    opt, opt_v = train_cifar10.build_optimizers(cfg, net, sampler, v)
    assert [g["lr"] for g in opt.param_groups] == [1e-5, 1e-7]
    assert len(opt.param_groups[0]["params"]) == 1 and opt.param_groups[0]["params"][0] is net.log_betas
    assert len(opt.param_groups[1]["params"]) == len(list(net.parameters())) - 1
    assert [g["lr"] for g in opt_v.param_groups] == [2e-5]
    trainer = dxmi_config.instantiate(cfg.trainer, batchsize=cfg.training.batchsize)
    assert type(trainer).__name__ == "DxMI_Trainer" and trainer.tau1 == 0.1 and trainer.tau2 == 0.01


def test_train_image_large_config_to_optimizer_groups_dry_run(tmp_path):
    """No GPU: the imagenet64_T10 YAML files (network shrunk by overrides, as `--diffusion.num_channels 32` would) ->
    MixedPrecisionTrainer masters + the RAdam groups of train_image_large.py:152-168."""
    import dxmi_config
    import train_image_large
    from models.cm.script_util import create_model_and_diffusion
    cfg = train_image_large.load_config(*_write_config_files(tmp_path, "imagenet64_T10"),
                                        {"diffusion": {"num_channels": 32, "num_res_blocks": 1, "num_head_channels": 16}})
    assert cfg.training.lr == 1e-8 and cfg.training.initial_log_loss_scale == 20 and cfg.data.name == "imagenet64"
    unet, _ = create_model_and_diffusion(**cfg.diffusion)
    unet.register_parameter("log_betas", torch.nn.Parameter(torch.zeros(cfg.sampler.n_timesteps)))
    v = dxmi_config.instantiate(cfg.value)
    mp, opt, opt_v = train_image_large.build_optimizers(cfg, unet, v)
    assert [g["lr"] for g in opt.param_groups] == [1e-8, 1e-6] and [g["lr"] for g in opt_v.param_groups] == [1e-5]
    assert opt.param_groups[1]["params"][0].numel() == 10 and mp.lg_loss_scale == 20


def test_fast_parameters_matches_module_parameters():
    """ops.fast_parameters (the weight-pack cache keys and the autograd argument lists of the HIP nets) yields exactly
    `module.parameters()`, in its order, also for a parameter registered on the net after the first call (the samplers add
    `log_betas` to a finished net, reference var_sampler.py / openai_diffusion.py)."""
    import torch
    from dxmi_hip import ops
    from models.DxMI.unet_small import Model
    net = Model(ch=32, out_ch=3, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[16], dropout=0.0, in_channels=3, resolution=32)
    a, b = list(ops.fast_parameters(net)), list(net.parameters())
    assert len(a) == len(b) and all(x is y for x, y in zip(a, b))
    net.log_betas = torch.nn.Parameter(torch.zeros(10))
    net.mid.block_1.conv1.weight = torch.nn.Parameter(torch.zeros_like(net.mid.block_1.conv1.weight))      # replaced, not updated
    a, b = list(ops.fast_parameters(net)), list(net.parameters())
    assert len(a) == len(b) and all(x is y for x, y in zip(a, b))
