"""Generators for the `generator=` argument of karras_sample, the sample_* / iterative_* functions and generate_large.py (the
reference's models/cm/random_util.py interface).

    g = get_generator("determ-indiv", num_samples=50000, seed=0)
    for b in range(n_batches):
        g.set_done_samples(b * batch * world)
        x = karras_sample(..., generator=g)

`dummy` forwards to torch.  `determ` and `determ-indiv` exist for one property: image i of a run sees the same noise whatever the
batch size and however many ranks share the run.  The reference gets it from one [num_samples, C, H, W] draw per call that it slices
(`determ`), or from num_samples torch generators and one randn launch per image (`determ-indiv`); their only difference is memory.
Here both ride one counter-based generator on the device (dxmi_randn_indexed / dxmi_randint_indexed, include/dxmi_hip.h): a normal
is a pure function of (seed, global sample index, draw number, element index) and a draw for the whole batch is one launch, so
`determ` and `determ-indiv` give the SAME stream.  It is this package's own stream, not torch's.

Row k of a call has the global index min(done_samples + rank + k * world, num_samples - 1) (the reference's arange + clamp); the
draw number counts the calls since the last set_done_samples / set_seed, randn and randint sharing one counter: image i's draw d is
the same noise whichever batch carries it, provided every batch makes the same sequence of calls (the samplers do).  The draws are
made on the device only: a CPU target raises DxmiError (no CPU fallback)."""
import torch
import torch.distributed as dist

from dxmi_hip import ops
from dxmi_hip._lib import DxmiError


def get_generator(generator, num_samples=0, seed=0):
    if generator == "dummy":
        return DummyGenerator()
    elif generator == "determ":
        return DeterministicGenerator(num_samples, seed)
    elif generator == "determ-indiv":
        return DeterministicIndividualGenerator(num_samples, seed)
    else:
        raise NotImplementedError


def sampling_generator(what, generator, noise=None):
    """What a DxMI sampler (VARSampler, OpenAIDiffusion, sample_guidance) draws with: None for no generator or a DummyGenerator (the
    sampler's own torch draws), else the generator.  Noise is injected or generated, not both."""
    if generator is not None and noise is not None:
        raise ValueError(f"{what}: noise= and generator= exclude each other")
    return None if isinstance(generator, DummyGenerator) else generator


def draw_controls(generator, n):
    """The next n draw numbers of a DeterministicGenerator as n control blocks (unused, draw, seed low word, seed high word): the
    host input of n captured launches that make their own noise (dxmi_var_step_fwd_indexed, dxmi_edm_step_fwd_indexed)."""
    seed = int(generator.seed) & ((1 << 64) - 1)
    out = []
    for _ in range(n):
        out += [0, generator._next_draw() & 0xFFFFFFFF, seed & 0xFFFFFFFF, seed >> 32]
    return out


class DummyGenerator:
    def randn(self, *args, **kwargs):
        return torch.randn(*args, **kwargs)

    def randint(self, *args, **kwargs):
        return torch.randint(*args, **kwargs)

    def randn_like(self, *args, **kwargs):
        return torch.randn_like(*args, **kwargs)


class DeterministicGenerator:
    """Noise for num_samples samples that depends on neither the batch size nor the number of ranks (see the module docstring).
    rank / world_size: torch.distributed's when it is initialised, else 0 and 1; give them to stand for one rank of a run without
    a process group."""

    def __init__(self, num_samples, seed=0, rank=None, world_size=None):
        if rank is None or world_size is None:
            init = dist.is_available() and dist.is_initialized()
            rank = (dist.get_rank() if init else 0) if rank is None else rank
            world_size = (dist.get_world_size() if init else 1) if world_size is None else world_size
        if num_samples < 1 or world_size < 1 or not 0 <= rank < world_size:
            raise ValueError(f"need num_samples >= 1 and 0 <= rank < world_size, got {num_samples}, {rank}, {world_size}")
        self.rank, self.world_size = int(rank), int(world_size)
        self.num_samples = int(num_samples)
        self.done_samples = 0
        self.seed = int(seed)
        self.draw = 0
        self._index = {}

    def get_indices(self, batch, device):
        """int64 [batch] on `device`: the global index of every row, cached until done_samples changes."""
        key = (int(batch), torch.device(device))
        idx = self._index.get(key)
        if idx is None:
            start = self.done_samples + self.rank
            idx = torch.arange(start, self.done_samples + self.world_size * key[0], self.world_size, dtype=torch.int64, device=key[1])
            idx = torch.clamp(idx, 0, self.num_samples - 1)
            assert len(idx) == key[0], f"rank={self.rank}, ws={self.world_size}, l={len(idx)}, bs={key[0]}"
            self._index[key] = idx
        return idx

    def _next_draw(self):
        d = self.draw
        self.draw += 1
        return d

    @staticmethod
    def _device(device):
        if device is not None:
            return torch.device(device)
        if not torch.cuda.is_available():
            raise DxmiError("the deterministic generators draw only on the HIP device path (no CPU fallback)")
        return torch.device("cuda", torch.cuda.current_device())

    def randn(self, *size, dtype=torch.float, device=None):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        idx = self.get_indices(size[0], self._device(device))
        z = ops.randn_indexed(idx, size[1:], self.seed, self._next_draw())
        return z if dtype == torch.float32 else z.to(dtype)

    def randint(self, low, high, size, dtype=torch.long, device=None):
        idx = self.get_indices(size[0], self._device(device))
        v = ops.randint_indexed(idx, tuple(size)[1:], low, high, self.seed, self._next_draw())
        return v if dtype == torch.int64 else v.to(dtype)

    def randn_like(self, tensor):
        return self.randn(*tensor.size(), dtype=tensor.dtype, device=tensor.device)

    def set_done_samples(self, done_samples):
        self.done_samples = int(done_samples)
        self.draw = 0
        self._index = {}

    def get_seed(self):
        return self.seed

    def set_seed(self, seed):
        self.seed = int(seed)
        self.draw = 0


class DeterministicIndividualGenerator(DeterministicGenerator):
    """The reference keeps one torch generator per sample here, seeded i + num_samples * seed, to save the memory of `determ`'s full
    draw.  With a counter-based generator that pair is the counter's index i under the key `seed`: the same stream as
    DeterministicGenerator, at the same (constant) memory."""
