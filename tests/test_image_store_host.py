"""CPU: dxmi_hip.data.ImageStore (the real-image dataset of the training scripts) without the library — the two normalisations
against the reference's expressions over every byte value, flips and layout, the order and coverage of an epoch over 1 - 3 ranks,
repeatability, seek / state, labels travelling with their images, the host-resident prefetch thread on CPU tensors, the file errors,
each script's loader selection and flag exclusion, and make_npz.py --labels_from_names."""
import struct
import threading
import zlib

import numpy as np
import pytest
import torch

from dxmi_hip.data import NORM_ADM, NORM_TOTENSOR, ImageStore, flip_seed, form_batch, normalise

M = 41


def _images(m=M, h=6, w=5, c=3, seed=0):
    """uint8 [m, h, w, c] with the row number in pixel (0, 0, 0) and in the labels."""
    arr = np.random.default_rng(seed).integers(0, 256, (m, h, w, c), dtype=np.uint8)
    arr[:, 0, 0, 0] = np.arange(m)
    return arr, np.arange(m, dtype=np.int64)


@pytest.fixture(scope="module")
def npz(tmp_path_factory):
    arr, lab = _images()
    p = tmp_path_factory.mktemp("store") / "img.npz"
    np.savez(p, arr, lab)
    return str(p), arr, lab


def _row_of(images, norm=NORM_ADM):
    """The source row of each image of a batch, from pixel (0, 0, 0) of the unflipped image or pixel (0, W-1, 0) of the mirrored one:
    returned for both readings."""
    inv = (images + 1) * 127.5 if norm == NORM_ADM else (images + 1) / 2 * 255
    return inv[:, 0, 0, 0].round().long(), inv[:, 0, 0, -1].round().long()


def test_norms_bitwise_over_every_byte():
    u8 = np.arange(256, dtype=np.uint8)
    adm = u8.astype(np.float32) / 127.5 - 1
    assert adm.dtype == np.float32
    assert torch.equal(normalise(torch.from_numpy(u8), NORM_ADM), torch.from_numpy(adm))
    assert torch.equal(normalise(torch.from_numpy(u8), "adm"), torch.from_numpy(adm))
    tot = 2 * torch.from_numpy(u8).float().div(255) - 1
    assert torch.equal(normalise(torch.from_numpy(u8), NORM_TOTENSOR), tot)
    # through a store: one image row holds every byte value
    assert adm[0] == -1 and adm[255] == 1 and tot[0] == -1 and tot[255] == 1


def test_flip_and_layout(npz):
    path, arr, _ = npz
    u8 = torch.from_numpy(arr[:4])
    plain = form_batch(u8, None, NORM_ADM)
    assert plain.shape == (4, 3, 6, 5) and plain.dtype == torch.float32 and plain.is_contiguous()
    assert torch.equal(plain, torch.from_numpy(arr[:4].astype(np.float32) / 127.5 - 1).permute(0, 3, 1, 2))
    mixed = form_batch(u8, torch.tensor([1, 0, 1, 0], dtype=torch.uint8), NORM_ADM)
    for i, f in enumerate([1, 0, 1, 0]):
        src = arr[i][:, ::-1] if f else arr[i]              # image_datasets.py:115-116
        assert torch.equal(mixed[i], torch.from_numpy(np.transpose(src.astype(np.float32) / 127.5 - 1, [2, 0, 1]).copy()))
    # a store with flips: every image is the plain or the mirrored source row, per the stated bits
    s = ImageStore(path, "cpu", NORM_ADM, batch_size=4, seed=3)
    rows, flips = s.plan(0)
    assert flips.dtype == torch.uint8 and 0 < int(flips.sum()) < len(flips)
    want = (torch.rand(M, generator=torch.Generator().manual_seed(flip_seed(3, 0, 0))) < 0.5)
    assert torch.equal(flips.bool(), want)
    for b, (x, y) in enumerate(s.epoch(0)):
        assert y is None
        assert torch.equal(x, form_batch(torch.from_numpy(arr[rows[4 * b:4 * b + 4].numpy()]), flips[4 * b:4 * b + 4], NORM_ADM))


@pytest.mark.parametrize("world", [1, 2, 3])
def test_epoch_coverage_and_order(npz, world):
    path, arr, lab = npz
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(7 + 0))
    seen = []
    for r in range(world):
        s = ImageStore(path, "cpu", NORM_ADM, batch_size=4, rank=r, world=world, seed=7, class_cond=True)
        assert s.batches_per_epoch == M // world // 4
        got = []
        for x, y in s.epoch(0):
            assert x.shape == (4, 3, 6, 5) and y.shape == (4,) and y.dtype == torch.int64
            a, b = _row_of(x)
            _, flips = s.plan(0)
            fl = flips[len(got):len(got) + 4].bool()
            assert torch.equal(torch.where(fl, b, a), y)           # the label is the row stored in the image's own pixel
            got += y.tolist()
        assert len(got) == (M // world // 4) * 4
        assert got == perm[r::world][:M // world][:len(got)].tolist()
        seen += got
        # another epoch is another order; the same (seed, epoch, rank) repeats bit for bit
        e1 = [y.tolist() for _, y in s.epoch(1)]
        assert sum(e1, []) != got
        again = list(s.epoch(0))
        s2 = ImageStore(path, "cpu", NORM_ADM, batch_size=4, rank=r, world=world, seed=7, class_cond=True)
        for (x1, y1), (x2, y2) in zip(again, s2.epoch(0)):
            assert torch.equal(x1, x2) and torch.equal(y1, y2)
    assert len(set(seen)) == len(seen) == world * (M // world // 4) * 4


def test_batches_state_and_seek(npz):
    path, _, _ = npz
    s = ImageStore(path, "cpu", NORM_TOTENSOR, batch_size=4, rank=1, world=2, seed=1, class_cond=True)
    n = s.batches_per_epoch
    assert n == 5
    it = s.batches()
    first = [next(it) for _ in range(n + 2)]                    # across the epoch boundary
    st = s.state()
    assert st == {"epoch": 1, "batch": 2}
    nxt = next(it)
    flat = [(x, c["y"]) for x, c in first]
    want = list(s.epoch(0)) + list(s.epoch(1))[:2]
    for (x1, y1), (x2, y2) in zip(flat, want):
        assert torch.equal(x1, x2) and torch.equal(y1, y2)
    s2 = ImageStore(path, "cpu", NORM_TOTENSOR, batch_size=4, rank=1, world=2, seed=1, class_cond=True)
    s2.seek(**st)
    res = next(s2.batches())
    assert torch.equal(res[0], nxt[0]) and torch.equal(res[1]["y"], nxt[1]["y"])
    assert s2.state() == {"epoch": 1, "batch": 3}
    # the last batch of an epoch rolls the position over
    s2.seek(0, n - 1)
    next(s2.batches())
    assert s2.state() == {"epoch": 1, "batch": 0}
    # without class_cond the labels stay behind
    s3 = ImageStore(path, "cpu", NORM_ADM, batch_size=4)
    x, cond = next(s3.batches())
    assert cond == {} and next(s3.epoch(0))[1] is None
    assert next(s3.batches(start_epoch=2))[0].shape == (4, 3, 6, 5)


@pytest.mark.parametrize("suffix", ["npz", "npy"])
def test_host_resident_path_matches_in_memory(npz, tmp_path, suffix):
    path, arr, lab = npz
    if suffix == "npy":
        path = str(tmp_path / "img.npy")
        np.save(path, arr)
        np.save(path + ".labels.npy", lab)
    before = threading.active_count()
    kw = dict(batch_size=4, rank=0, world=2, seed=5, class_cond=True)
    mem = ImageStore(path, "cpu", NORM_ADM, resident="device", **kw)
    host = ImageStore(path, "cpu", NORM_ADM, resident="host", **kw)
    assert mem.resident == "device" and host.resident == "host"
    assert ImageStore(path, "cpu", NORM_ADM, resident="auto", device_budget_bytes=10, **kw).resident == "host"
    assert ImageStore(path, "cpu", NORM_ADM, resident="auto", **kw).resident == "device"
    a, b = mem.batches(), host.batches()
    for _ in range(2 * mem.batches_per_epoch + 1):                # across the epoch boundary, twice
        (x1, c1), (x2, c2) = next(a), next(b)
        assert torch.equal(x1, x2) and torch.equal(c1["y"], c2["y"])
    assert mem.state() == host.state()
    for (x1, y1), (x2, y2) in zip(mem.epoch(3), host.epoch(3)):
        assert torch.equal(x1, x2) and torch.equal(y1, y2)
    assert any(t.name == "dxmi-image-store" for t in threading.enumerate())      # b's feeder is still running
    host.close()
    assert not any(t.name == "dxmi-image-store" for t in threading.enumerate())
    assert threading.active_count() == before
    # an abandoned iterator ends its thread when it is collected
    it = host.batches()
    next(it)
    del it
    import gc
    gc.collect()
    assert not any(t.name == "dxmi-image-store" for t in threading.enumerate())


def test_file_errors(tmp_path):
    arr, lab = _images()
    kw = dict(batch_size=4)

    def save(name, *a):
        p = str(tmp_path / name)
        np.savez(p, *a)
        return p

    with pytest.raises(ValueError, match=r"float.npz.*float32"):
        ImageStore(save("float.npz", arr.astype(np.float32)), "cpu", NORM_ADM, **kw)
    with pytest.raises(ValueError, match=r"rank3.npz.*\(41, 6, 5\)"):
        ImageStore(save("rank3.npz", arr[..., 0]), "cpu", NORM_ADM, **kw)
    with pytest.raises(ValueError, match=r"nolab.npz.*class_cond"):
        ImageStore(save("nolab.npz", arr), "cpu", NORM_ADM, class_cond=True, **kw)
    with pytest.raises(ValueError, match=r"short.npz.*40 labels for 41 images"):
        ImageStore(save("short.npz", arr, lab[:40]), "cpu", NORM_ADM, class_cond=True, **kw)
    with pytest.raises(ValueError, match=r"nolab.npz.*13 per rank.*16"):
        ImageStore(str(tmp_path / "nolab.npz"), "cpu", NORM_ADM, batch_size=16, world=3, rank=2)
    np.save(str(tmp_path / "f.npy"), arr.astype(np.float64))
    with pytest.raises(ValueError, match=r"f.npy.*float64"):
        ImageStore(str(tmp_path / "f.npy"), "cpu", NORM_ADM, **kw)
    assert ImageStore(save("ok.npz", arr, lab.astype(np.int32)), "cpu", NORM_ADM, class_cond=True, **kw).has_labels


def test_scripts_exclude_synthetic_and_real(capsys):
    import cm_train
    import train_cifar10
    import train_image_large
    for mod, argv in ((cm_train, ["--synthetic_data", "True", "--data_npz", "x.npz"]),
                      (train_cifar10, ["--config", "builtin:cifar10_T10", "--dataset", "builtin", "--synthetic_data", "--data_npz", "x.npz"]),
                      (train_image_large, ["--config", "c", "--dataset", "d", "--run", "r", "--synthetic_data", "--data_npz", "x.npz"])):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(argv)
        assert e.value.code == 2
        assert "exclude each other" in capsys.readouterr().err
    # each alone parses
    assert cm_train.parse_args(["--data_npz", "x.npz"]).data_npz == "x.npz"
    assert cm_train.parse_args(["--synthetic_data", "True"]).data_npz == ""
    assert cm_train.parse_args([]).data_resident == "auto"
    with pytest.raises(NotImplementedError, match="--data_npz"):
        cm_train.make_loader(cm_train.parse_args([]), "cpu", 0, 1)


def test_loader_selection_of_each_script(tmp_path):
    import cm_train
    import train_cifar10
    import train_image_large
    arr, lab = _images(48, 32, 32)
    p = str(tmp_path / "tiny.npz")
    np.savez(p, arr, lab)

    a = cm_train.parse_args(["--data_npz", p, "--batch_size", "6", "--class_cond", "True", "--seed", "9", "--data_resident", "host"])
    data, store = cm_train.make_loader(a, "cpu", 1, 2)
    assert isinstance(store, ImageStore) and store.norm == NORM_ADM and store.batch_size == 6 and (store.rank, store.world) == (1, 2)
    assert store.seed == 9 and store.resident == "host" and store.with_labels
    x, cond = next(data)
    assert x.shape == (6, 3, 32, 32) and cond["y"].shape == (6,)
    line = store.describe()
    for piece in (p, "48 images", "32x32x3", "labels yes", "resident host", "4 batches"):
        assert piece in line, line
    store.close()
    syn, none = cm_train.make_loader(cm_train.parse_args(["--synthetic_data", "True", "--image_size", "8", "--batch_size", "2"]), "cpu", 0, 1)
    assert none is None and next(syn)[0].shape == (2, 3, 8, 8)

    args, unknown = train_cifar10.parse_args(["--config", "builtin:cifar10_T10", "--dataset", "builtin", "--data_npz", p,
                                               "--training.batchsize", "16"])
    import cmd_utils as cmd
    cfg = train_cifar10.load_config(args.config, args.dataset, cmd.parse_nested_args(cmd.parse_unknown_args(unknown)))
    store = train_cifar10.make_store(args, cfg, "cpu", 0, 2)
    assert store.norm == NORM_TOTENSOR and store.batch_size == 8 and store.world == 2 and store.seed == cfg.training.seed
    assert not store.with_labels and store.resident == "device"
    x, y = next(iter(train_cifar10.make_loader(args, cfg, "cpu", 0, 2, 0, store)))
    assert x.shape == (8, 3, 32, 32) and y is None and x.min() >= -1 and x.max() <= 1
    args.data_npz = ""
    assert train_cifar10.make_store(args, cfg, "cpu", 0, 2) is None
    args.synthetic_data, args.max_iters = True, 2
    assert len(list(train_cifar10.make_loader(args, cfg, "cpu", 0, 2, 0))) == 2

    args, unknown = train_image_large.parse_args(["--config", "builtin:imagenet64_T10", "--dataset", "builtin", "--run", "r", "--data_npz", p,
                                                   "--training.batchsize", "8"])
    cfg = train_image_large.load_config(args.config, args.dataset, cmd.parse_nested_args(cmd.parse_unknown_args(unknown)))
    data, store = train_image_large.make_loader(args, cfg, "cpu", 1, 2)
    want_cc = bool(cfg.data.get("class_cond", cfg.sampler.get("class_cond", False)))
    assert store.norm == NORM_ADM and store.batch_size == 4 and (store.rank, store.world) == (1, 2) and store.with_labels == want_cc
    x, cond = next(data)
    assert x.shape == (4, 3, 32, 32) and (("y" in cond) == want_cc)


def _write_png(path, img):
    """8-bit RGB, filter 0: what make_npz.py decodes without PIL."""
    h, w, _ = img.shape
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw))
                + chunk(b"IEND", b""))


def test_make_npz_labels_from_names(tmp_path):
    import make_npz
    d = tmp_path / "png"
    d.mkdir()
    names = ["b_0.png", "a_1.png", "c_2.png", "a_3.png", "b_4.png", "c_5.png"]
    rng = np.random.default_rng(1)
    imgs = {n: rng.integers(0, 256, (4, 4, 3), dtype=np.uint8) for n in names}
    for n, im in imgs.items():
        _write_png(str(d / n), im)
    make_npz.main(["--dir", str(d), "--out", str(tmp_path / "lab.npz"), "--labels_from_names"])
    z = np.load(tmp_path / "lab.npz")
    assert z.files == ["arr_0", "arr_1"]
    assert z["arr_0"].shape == (6, 4, 4, 3) and z["arr_0"].dtype == np.uint8
    assert z["arr_1"].tolist() == [1, 0, 2, 0, 1, 2] and z["arr_1"].dtype == np.int64      # files in index order, classes a < b < c
    for i, n in enumerate(names):
        assert np.array_equal(z["arr_0"][i], imgs[n])
    make_npz.main(["--dir", str(d), "--out", str(tmp_path / "plain.npz")])
    assert np.load(tmp_path / "plain.npz").files == ["arr_0"]
    s = ImageStore(str(tmp_path / "lab.npz"), "cpu", NORM_ADM, batch_size=2, class_cond=True)
    assert s.has_labels and s.image_shape == (4, 4, 3)
