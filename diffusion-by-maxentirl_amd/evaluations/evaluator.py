"""The ADM sample-quality evaluator on the device: `python evaluations/evaluator.py REF_BATCH.npz SAMPLE_BATCH.npz` prints

    Inception Score: ...
    FID: ...
    sFID: ...
    Precision: ...
    Recall: ...

as the reference's TensorFlow evaluator does (evaluations/evaluator.py:27-59 there), for the `arr_0` uint8 [N, H, W, 3] batches
`make_npz.py` writes.  The flow is the reference's; every heavy step runs in the HIP library:

    activations   the extractor (`--extractor module:attr`, default pytorch_fid.inception:EvalInceptionV3) over batches of
                  `--batch_size` images streamed from the .npz (host memory stays one batch): pool [N, 2048], spatial [N, 2023]
    statistics    a batch carrying mu / sigma / mu_s / sigma_s uses them (read_statistics); otherwise dxmi_fid_stats (the spatial
                  features padded by one zero column on the device: D % 4 == 0, that row / column dropped on the host)
    IS            dxmi_inception_score on the sample pool features and the extractor's softmax_weight (splits of 5000)
    FID / sFID    pytorch_fid.fid_score.calculate_frechet_distance (the reference's float64 sqrtm algorithm)
    P / R         dxmi_knn_radii (k = 3) of both sets, then dxmi_pr_membership

Two metrics the reference evaluator does not have are printed after `Recall:` when asked for, on the same pool features:

    --kid         KID: / KID std: the Kernel Inception Distance (Binkowski et al. 2018), the unbiased MMD^2 estimate with the kernel
                  (x . y / D + 1)^3: mean and standard deviation over `--kid_subsets` (100) subsets of `--kid_subset_size` (1000)
                  rows of each set drawn with `--kid_seed` (0); `--kid_subsets 0`: one estimate over all rows (std 0).  Unlike FID
                  it has no bias in the sample count, so a 10 000-image number and a 50 000-image number can be compared.
                  dxmi_kid_sums: all subsets in one launch, the sums in fp64
    --prdc        Density: / Coverage: (Naeem et al. 2020) with `--dc_k` (5) nearest neighbours: dxmi_knn_radii of the reference
                  set, then dxmi_dc_counts (how many samples fall strictly inside each reference ball); density = sum / (k NB),
                  coverage = the fraction of reference balls that hold a sample.  Robust where precision / recall follow outliers

Not pinned to the TensorFlow numbers: the reference graph resizes with TF's legacy bilinear and normalises (x - 128) / 128, this
extractor follows pytorch_fid and runs in bf16, and the weight file is not in this image.  The five numbers are comparable to the
reference evaluator's, not equal to them.  Out of scope: clamp_to_percentile, realism scores and nearest indices
(ManifoldEstimator.evaluate; the reference CLI never uses them), and sharding an evaluation over several GPUs.
Single process, one device; there is no CPU path.
"""
import argparse
import os
import sys
import zipfile
from contextlib import contextmanager

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

DEFAULT_EXTRACTOR = "pytorch_fid.inception:EvalInceptionV3"
NHOOD_K = 3                 # ManifoldEstimator(nhood_sizes=(3,))
IS_SPLIT = 5000             # compute_inception_score(split_size=5000)
UNPINNED_NOTE = ("note: the Inception extractor is unpinned (pytorch_fid resize / normalisation, bf16 convolutions): the numbers "
                 "are comparable to the TensorFlow evaluator's, not bit-identical")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="IS / FID / sFID / precision / recall of a sample batch against a reference batch")
    ap.add_argument("ref_batch", help="path to reference batch npz file")
    ap.add_argument("sample_batch", help="path to sample batch npz file")
    ap.add_argument("--extractor", default=DEFAULT_EXTRACTOR, help="feature extractor 'module:attr' (class or instance)")
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--kid", action="store_true", help="also print the Kernel Inception Distance (KID: / KID std:)")
    ap.add_argument("--kid_subsets", type=int, default=100, help="number of KID subsets (0: one estimate over all rows)")
    ap.add_argument("--kid_subset_size", type=int, default=1000, help="rows of each set per KID subset")
    ap.add_argument("--kid_seed", type=int, default=0, help="seed of the KID subset draw")
    ap.add_argument("--prdc", action="store_true", help="also print density and coverage (Density: / Coverage:)")
    ap.add_argument("--dc_k", type=int, default=5, help="nearest neighbours of the density / coverage radii")
    a = ap.parse_args(argv)
    if a.batch_size < 1:
        ap.error("--batch_size must be >= 1")
    if a.kid_subsets < 0 or a.kid_subset_size < 2:
        ap.error("--kid_subsets must be >= 0 and --kid_subset_size >= 2")
    if a.dc_k < 1:
        ap.error("--dc_k must be >= 1")
    return a


# ------------------------------------------------------------------------------------------------ streaming .npz reader
class NpzArrayReader:
    """Batches of one array of an .npz without loading it: the member's .npy header through numpy.lib.format, then the rows
    read straight from the (possibly deflated) zip member.  Fortran-ordered or object arrays fall back to np.load."""

    def __init__(self, f, shape, dtype, path, arr=None):
        self.f, self.shape, self.dtype, self.path, self.arr = f, tuple(shape), dtype, path, arr
        self.idx = 0

    def __len__(self):
        return self.shape[0] if self.shape else 0

    def read_batch(self, batch_size):
        n = len(self) - self.idx
        if n <= 0:
            return None
        bs = min(batch_size, n)
        if self.arr is not None:
            out = self.arr[self.idx:self.idx + bs]
        else:
            count = bs * int(np.prod(self.shape[1:], dtype=np.int64))
            nbytes = count * self.dtype.itemsize
            data = self.f.read(nbytes)
            if len(data) != nbytes:
                raise ValueError(f"{self.path}: truncated array data (wanted {nbytes} bytes, got {len(data)})")
            out = np.frombuffer(data, dtype=self.dtype).reshape((bs,) + self.shape[1:])
        self.idx += bs
        return out

    def batches(self, batch_size):
        while True:
            b = self.read_batch(batch_size)
            if b is None:
                return
            yield b


@contextmanager
def open_npz_array(path, name="arr_0"):
    with zipfile.ZipFile(path, "r") as z:
        member = f"{name}.npy"
        if member not in z.namelist():
            raise ValueError(f"{path}: no {name} in the npz file")
        with z.open(member, "r") as f:
            version = np.lib.format.read_magic(f)
            if version == (1, 0):
                shape, fortran, dtype = np.lib.format.read_array_header_1_0(f)
            elif version == (2, 0):
                shape, fortran, dtype = np.lib.format.read_array_header_2_0(f)
            else:
                shape, fortran, dtype = None, True, None
            if fortran or dtype is None or dtype.hasobject:
                arr = np.load(path)[name]
                yield NpzArrayReader(None, arr.shape, arr.dtype, path, arr=arr)
            else:
                yield NpzArrayReader(f, shape, dtype, path)


def check_image_batch(reader):
    """arr_0 must be uint8 [N, H, W, 3] with N >= NHOOD_K + 1 (the k-NN radii need k + 1 rows)."""
    shape, dtype = reader.shape, reader.dtype
    if len(shape) != 4 or shape[3] != 3:
        raise ValueError(f"{reader.path}: arr_0 must be NHWC images [N, H, W, 3], got shape {shape}")
    if dtype != np.uint8:
        raise ValueError(f"{reader.path}: arr_0 must be uint8 in [0, 255], got {dtype}")
    if shape[0] < NHOOD_K + 1:
        raise ValueError(f"{reader.path}: {shape[0]} images; precision / recall need at least {NHOOD_K + 1}")


def read_precomputed_statistics(path):
    """(mu, sigma, mu_s, sigma_s) float64 when the batch carries them (reference read_statistics), else None."""
    with np.load(path) as obj:
        keys = set(obj.keys())
        if "mu" not in keys:
            return None
        missing = {"sigma", "mu_s", "sigma_s"} - keys
        if missing:
            raise ValueError(f"{path}: has mu but not {sorted(missing)}")
        return tuple(np.asarray(obj[k], dtype=np.float64) for k in ("mu", "sigma", "mu_s", "sigma_s"))


# ------------------------------------------------------------------------------------------------ device flow
def read_activations(path, extractor, batch_size, device="cuda"):
    """(pool fp32 [N, P], spatial fp32 [N, S4]) on the device; the spatial rows are padded with zeros to S4 = S rounded up to a
    multiple of 4 (dxmi_fid_stats needs D % 4 == 0).  Returns (pool, spatial_padded, S)."""
    import torch
    with open_npz_array(path) as reader:
        check_image_batch(reader)
        N = len(reader)
        pool = spatial = None
        S = 0
        start = 0
        for batch in reader.batches(batch_size):
            x = torch.from_numpy(np.array(batch, copy=True)).to(device)          # frombuffer views are read-only
            p, s = extractor(x)
            p, s = p.reshape(p.shape[0], -1).float(), s.reshape(s.shape[0], -1).float()
            if p.shape[0] != x.shape[0] or s.shape[0] != x.shape[0]:
                raise ValueError(f"{path}: the extractor returned {p.shape[0]} / {s.shape[0]} rows for {x.shape[0]} images")
            if pool is None:
                S = s.shape[1]
                pool = torch.empty((N, p.shape[1]), dtype=torch.float32, device=device)
                spatial = torch.zeros((N, (S + 3) // 4 * 4), dtype=torch.float32, device=device)
            if not (bool(torch.isfinite(p).all()) and bool(torch.isfinite(s).all())):
                raise ValueError(f"{path}: non-finite activations in images {start}..{start + x.shape[0] - 1}")
            pool[start:start + x.shape[0]] = p
            spatial[start:start + x.shape[0], :S] = s
            start += x.shape[0]
    return pool, spatial, S


def statistics(path, pool, spatial, S):
    from pytorch_fid.fid_score import activation_statistics
    pre = read_precomputed_statistics(path)
    if pre is not None:
        return pre
    mu, sigma = activation_statistics(pool)
    mu_s, sigma_s = activation_statistics(spatial)
    return mu, sigma, mu_s[:S], sigma_s[:S, :S]


def precision_recall(ref_pool, sample_pool, k=NHOOD_K):
    """(precision, recall) of Evaluator.compute_prec_recall: pr[0] is the mean of the SAMPLE flags (samples inside the reference
    manifold), pr[1] the mean of the reference flags."""
    from dxmi_hip import ops
    r_ref = ops.knn_radii(ref_pool, k)
    r_sample = ops.knn_radii(sample_pool, k)
    ref_in, sample_in = ops.pr_membership(ref_pool, r_ref, sample_pool, r_sample)
    return int(sample_in.sum()) / sample_in.numel(), int(ref_in.sum()) / ref_in.numel()


def kid_subset_indices(nx, ny, subsets, subset_size, seed):
    """The rows of the KID subsets: two int32 arrays [subsets, m], m = min(nx, ny, subset_size), drawn without replacement within
    a subset from one generator, for each subset in order its rows of the first set and then of the second."""
    m = min(nx, ny, subset_size)
    rng = np.random.default_rng(seed)
    ix, iy = np.empty((subsets, m), dtype=np.int32), np.empty((subsets, m), dtype=np.int32)
    for s in range(subsets):
        ix[s] = rng.choice(nx, m, replace=False)
        iy[s] = rng.choice(ny, m, replace=False)
    return ix, iy


def kernel_inception_distance(ref_pool, sample_pool, subsets=100, subset_size=1000, seed=0):
    """(mean, std) over the subsets of the unbiased MMD^2 estimate with k(u, v) = (u . v / D + 1)^3 (Binkowski et al. 2018):
    per subset (Sxx + Syy) / (m (m - 1)) - 2 Sxy / m^2 from ops.kid_sums, mean and np.std (ddof 0) on the host in float64.
    subsets=0: the one estimate over all rows of both sets, Sxx / (nx (nx - 1)) + Syy / (ny (ny - 1)) - 2 Sxy / (nx ny), std 0."""
    import torch
    from dxmi_hip import ops
    nx, ny = ref_pool.shape[0], sample_pool.shape[0]
    if min(nx, ny) < 2 or (subsets > 0 and subset_size < 2):
        raise ValueError(f"kernel_inception_distance: need at least 2 rows per set and per subset ({nx}, {ny}, subset_size {subset_size})")
    D = ref_pool.shape[1]
    if subsets == 0:
        sxx, syy, sxy = ops.kid_sums(ref_pool, sample_pool, gamma=1.0 / D, coef0=1.0).cpu().numpy()[0]
        return float(sxx / (nx * (nx - 1)) + syy / (ny * (ny - 1)) - 2.0 * sxy / (nx * ny)), 0.0
    ix, iy = kid_subset_indices(nx, ny, subsets, subset_size, seed)
    m = ix.shape[1]
    sums = ops.kid_sums(ref_pool, sample_pool, torch.from_numpy(ix).to(ref_pool.device), torch.from_numpy(iy).to(ref_pool.device),
                        gamma=1.0 / D, coef0=1.0).cpu().numpy()
    vals = (sums[:, 0] + sums[:, 1]) / (m * (m - 1)) - 2.0 * sums[:, 2] / (m * m)
    return float(np.mean(vals)), float(np.std(vals))


def density_coverage(ref_pool, sample_pool, k=5):
    """(density, coverage) of Naeem et al. 2020 as the `prdc` package computes them: with r_i the distance of reference row i to its
    k-th nearest other reference row and c_i the number of sample rows strictly inside that ball, density = sum_i c_i / (k NB)
    and coverage = mean_i (c_i > 0)."""
    from dxmi_hip import ops
    na, nb = ref_pool.shape[0], sample_pool.shape[0]
    if na < k + 1:
        raise ValueError(f"density_coverage: {na} reference rows; k = {k} needs at least {k + 1}")
    r = ops.knn_radii(ref_pool, k)
    c = ops.dc_counts(ref_pool, r, sample_pool)
    return int(c.sum()) / (k * nb), int((c > 0).sum()) / na


def evaluate(ref_batch, sample_batch, extractor, batch_size=64, kid=None, prdc=None, extra=None):
    """The five numbers, in the order they are printed.  kid: None or dict(subsets, subset_size, seed); prdc: None or dict(k);
    what they ask for goes into the dict `extra` under "kid" (mean, std) and "prdc" (density, coverage)."""
    import torch
    from dxmi_hip import ops
    from pytorch_fid.fid_score import calculate_frechet_distance
    ops.device_check()
    if (kid is not None or prdc is not None) and extra is None:
        raise ValueError("evaluate: kid / prdc need the dict `extra` to put their results into")
    w = getattr(extractor, "softmax_weight", None)
    if not (torch.is_tensor(w) and w.dim() == 2):
        raise ValueError("the extractor has no softmax_weight [2048, C] tensor (the Inception Score's classifier weight)")
    print("computing reference batch activations...")
    ref_pool, ref_spatial, S_ref = read_activations(ref_batch, extractor, batch_size)
    print("computing/reading reference batch statistics...")
    ref_stats = statistics(ref_batch, ref_pool, ref_spatial, S_ref)
    print("computing sample batch activations...")
    sample_pool, sample_spatial, S_sample = read_activations(sample_batch, extractor, batch_size)
    print("computing/reading sample batch statistics...")
    sample_stats = statistics(sample_batch, sample_pool, sample_spatial, S_sample)
    print("Computing evaluations...")
    wt = w.to(sample_pool.device).float().t().contiguous()                 # [C, 2048]: fc.weight layout
    inception_score = ops.inception_score(sample_pool, wt, IS_SPLIT)
    fid = calculate_frechet_distance(sample_stats[0], sample_stats[1], ref_stats[0], ref_stats[1])
    sfid = calculate_frechet_distance(sample_stats[2], sample_stats[3], ref_stats[2], ref_stats[3])
    prec, recall = precision_recall(ref_pool, sample_pool)
    if kid is not None:
        extra["kid"] = kernel_inception_distance(ref_pool, sample_pool, **kid)
    if prdc is not None:
        extra["prdc"] = density_coverage(ref_pool, sample_pool, **prdc)
    return inception_score, float(fid), float(sfid), prec, recall


def main(argv=None):
    a = parse_args(argv)
    from pytorch_fid.fid_score import load_extractor
    extractor = load_extractor(a.extractor)
    print(UNPINNED_NOTE)
    extra = {}
    inception_score, fid, sfid, prec, recall = evaluate(
        a.ref_batch, a.sample_batch, extractor, a.batch_size,
        kid=dict(subsets=a.kid_subsets, subset_size=a.kid_subset_size, seed=a.kid_seed) if a.kid else None,
        prdc=dict(k=a.dc_k) if a.prdc else None, extra=extra)
    print("Inception Score:", inception_score)
    print("FID:", fid)
    print("sFID:", sfid)
    print("Precision:", prec)
    print("Recall:", recall)
    if a.kid:
        print("KID:", extra["kid"][0])
        print("KID std:", extra["kid"][1])
    if a.prdc:
        print("Density:", extra["prdc"][0])
        print("Coverage:", extra["prdc"][1])
    return inception_score, fid, sfid, prec, recall


if __name__ == "__main__":
    main()
