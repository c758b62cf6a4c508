"""Sample realism by horizon: the Frechet distance between Gaussian fits of feature vectors of real and of sampled frames.

A *Frechet step* is a skill step (``ForecastSkill``'s plan: ``S`` sampled futures per row after a context of ``q`` observed frames, the
same noise keys) whose decoded frames are not scored against their targets but embedded: ``features="reader"`` takes the vision frames
through a ``DigitClassifier``'s trunk and ``fc1`` (``D = 128``), ``features="encoder"`` takes both modalities through the model's own
encoders (``D`` = the embedding size).  The target frames go through the same path once per ``(b, t)``.  Every row gets the bin of its
horizon -- ``obs`` (``h = 0``), then ``[e_i, e_{i+1})`` of ``edges``, the last bin open to ``T``, exactly ``SumTable._bin_slices``' bins
of ``ForecastSkill.horizon`` -- or -1 when its frame is dead or its horizon lies below the first edge.

**The statistic**, per stream, side (real, generated) and bin ``j``, in double: ``n_j`` (the rows of the bin), ``s_j = sum_n x_n``
``[D]`` and ``M_j = sum_n x_n x_n^T`` ``[D, D]`` (a full matrix, both triangles bit-identical) -- ``[J, 1 + D + D * D]`` doubles that
any number of steps add up in.  Every product is exact in double (24 + 24 bits).  ``FrechetDistance.reference_moments`` states it in
torch float64; ``mtrssm_feature_moments`` is the kernel (``FrechetDistance.fold``), used for GPU tensors: it reads the fp32 rows in
place (``ldx``: a padded buffer's row stride), masks per bin, and adds in an order fixed by ``(N, D, J)``.

**The distance**, on the host in float64 (``FrechetTable.compute``): ``mu = s / n``, ``Sigma = M / n - mu mu^T`` (symmetrised),

    fd = |mu_r - mu_g|^2 + tr Sigma_r + tr Sigma_g - 2 sum_i sqrt(lambda_i(Sigma_r^1/2 Sigma_g Sigma_r^1/2))

with ``Sigma_r^1/2`` and the ``lambda`` from ``eigh`` / ``eigvalsh``, negative eigenvalues clamped to 0 and ``fd`` clamped to ``>= 0``;
``trace_ratio = tr Sigma_g / tr Sigma_r`` (below 1: the samples are blurred or collapsed).  Fewer than 2 rows on a side give NaN.
"""

from __future__ import annotations

import torch
from torch import Tensor

from multimodal_mtrssm_amd import _lib
from multimodal_mtrssm_amd.skill import MODALITIES, ForecastSkill, ObservingConfig, SumTable

FEATURES = ("reader", "encoder")
PARTS = ("fd", "mean", "cov", "trace_ratio", "n")
SIDES = ("real", "generated")
MAX_DIM = 256
MAX_BINS = 16

_WS: dict[tuple[int, int], Tensor] = {}
_WS_CACHED_BYTES = 64 << 20  # a larger call takes a tensor of its own


def _workspace(device: torch.device, nbytes: int) -> Tensor:
    """The moment kernel's workspace on the current stream of ``device`` (float64 words, >= nbytes): one cached buffer per (device,
    stream) where it fits, grown on demand.  Calls on one stream run in order, so they can share it."""
    words = (nbytes + 7) // 8
    if nbytes > _WS_CACHED_BYTES:
        return torch.empty(words, dtype=torch.float64, device=device)
    key = (torch.device(device).index or 0, _lib.stream_ptr(device))
    ws = _WS.get(key)
    if ws is None or ws.numel() < words:
        ws = _WS[key] = torch.empty(words, dtype=torch.float64, device=device)
    return ws


def cells(dim: int) -> int:
    """The doubles of one bin: the count, the sum ``[D]`` and the second moment ``[D, D]``."""
    return 1 + dim + dim * dim


def bin_names(edges: tuple[int, ...]) -> tuple[str, ...]:
    """``(1, 2, 4, 8)`` -> ``("obs", "h1", "h2", "h4", "h8")``."""
    return ("obs", *(f"h{e}" for e in edges))


class FrechetDistance(ObservingConfig):
    """``FrechetDistance(q, samples=S, observe=..., features="reader", edges=(1, 2, 4, 8))``: every row observes ``q >= 1`` frames of
    ``observe``, then ``S`` sampled futures run open loop (``ForecastSkill``'s plan and noise); the decoded frames and the target frames
    are embedded by ``features`` and their moments are kept per horizon bin of ``edges``.  ``max_frames`` as ``ForecastSkill``'s."""

    def __init__(self, context: int, samples: int = 1, observe: str = "both", features: str = "reader",
                 edges: tuple[int, ...] = (1, 2, 4, 8)) -> None:
        skill = ForecastSkill(context, samples, observe)  # (its refusals are this config's)
        if features not in FEATURES:
            msg = f"features must be one of {FEATURES}, got {features!r}"
            raise ValueError(msg)
        if (isinstance(edges, (str, bytes)) or not isinstance(edges, (tuple, list)) or not edges or len(edges) >= MAX_BINS
                or any(isinstance(e, bool) or not isinstance(e, int) for e in edges) or edges[0] < 1
                or any(a >= b for a, b in zip(edges, edges[1:]))):  # noqa: RUF007
            msg = f"edges must be 1 .. {MAX_BINS - 1} ascending integer horizons >= 1, got {edges!r}"
            raise ValueError(msg)
        self.context, self.samples, self.observe = skill.context, skill.samples, skill.observe
        self.features, self.edges = features, tuple(edges)
        self.max_frames = skill.max_frames
        self.group = None  # the process group FrechetTable.all_reduce uses (FlatDataParallel.frechet binds it)

    def __repr__(self) -> str:
        return (f"FrechetDistance({self.context}, samples={self.samples}, observe={self.observe!r}, features={self.features!r}, "
                f"edges={self.edges})")

    @property
    def bin_names(self) -> tuple[str, ...]:
        return bin_names(self.edges)

    @property
    def streams(self) -> tuple[str, ...]:
        """The streams of frames that are embedded: the reader sees vision only, the model's encoders both modalities."""
        return ("vision",) if self.features == "reader" else MODALITIES

    def plan(self):  # noqa: ANN201
        """``ForecastSkill``'s plan: the same copies, the same noise keys -- the same futures can be scored by both."""
        return ForecastSkill(self.context, self.samples, self.observe).plan()

    def bins(self, batch: int, steps: int, valid: Tensor | None, device: torch.device) -> Tensor:
        """int32 ``[B, T]`` on ``device``: the bin of every frame (-1: dead, or a horizon below the first edge); nothing is read back."""
        context = torch.full((batch,), min(self.context, (1 << 31) - 1), dtype=torch.int32, device=device)
        h, live = ForecastSkill.horizon(context, valid, steps)
        edges = torch.tensor(self.edges, dtype=h.dtype, device=device)
        j = torch.bucketize(h, edges, right=True)  # h in [e_i, e_{i+1}) -> i + 1
        j = torch.where(h == 0, torch.zeros_like(j), torch.where(h < self.edges[0], torch.full_like(j, -1), j))
        return torch.where(live, j, torch.full_like(j, -1)).to(torch.int32)

    # -- the rule in torch, in float64 -------------------------------------------------------------------------------------------------
    @staticmethod
    def _checked(x: Tensor, bins: Tensor, J: int, table: Tensor) -> tuple[int, int]:  # noqa: N803
        if x.dim() != 2 or x.dtype != torch.float32 or x.numel() == 0 or (x.shape[1] > 1 and x.stride(1) != 1):  # noqa: PLR2004
            msg = f"x must be a non-empty float32 [N, D] tensor whose rows are contiguous, got {x.dtype} {tuple(x.shape)} strides {x.stride()}"
            raise ValueError(msg)
        n, d = x.shape
        if isinstance(J, bool) or not isinstance(J, int) or not 1 <= J <= MAX_BINS or not 1 <= d <= MAX_DIM:
            msg = f"need 1 <= J <= {MAX_BINS} and 1 <= D <= {MAX_DIM}, got J {J!r} and D {d}"
            raise ValueError(msg)
        if bins.dtype != torch.int32 or tuple(bins.shape) != (n,) or bins.device != x.device:
            msg = f"bins must be an int32 tensor of shape ({n},) on {x.device}, got {bins.dtype} {tuple(bins.shape)} on {bins.device}"
            raise ValueError(msg)
        want = (J, cells(d))
        if tuple(table.shape) != want or table.dtype != torch.float64 or not table.is_contiguous() or table.device != x.device:
            msg = f"table must be a contiguous float64 {want} buffer on {x.device}, got {table.dtype} {tuple(table.shape)} on {table.device}"
            raise ValueError(msg)
        return n, d

    @staticmethod
    def reference_moments(x: Tensor, bins: Tensor, J: int, table: Tensor) -> Tensor:  # noqa: N803
        """The rule in float64 on any device, in place: ``table[j] += (n_j, sum x, sum x x^T)`` over the rows with ``bins == j``; a
        row whose bin is outside ``[0, J)`` is skipped.  ``x`` may be a strided view of a padded buffer."""
        _, d = FrechetDistance._checked(x, bins, J, table)
        xd = x.to(torch.float64)
        zero = torch.zeros((), dtype=torch.float64, device=x.device)
        for j in range(J):
            mine = bins == j
            xs = torch.where(mine.unsqueeze(1), xd, zero)
            table[j, 0] += mine.sum().to(torch.float64)
            table[j, 1 : 1 + d] += xs.sum(0)
            table[j, 1 + d :] += (xs.t() @ xs).reshape(-1)
        return table

    # -- the kernel on the GPU, the rule elsewhere -------------------------------------------------------------------------------------
    @staticmethod
    def fold(x: Tensor, bins: Tensor, J: int, table: Tensor) -> Tensor:  # noqa: N803
        """One ``mtrssm_feature_moments`` call (two launches, nothing read back) on torch's current stream; non-GPU tensors take
        ``reference_moments``.  ``x`` is read in place with its row stride; ``table`` is added onto and returned."""
        n, d = FrechetDistance._checked(x, bins, J, table)
        if not x.is_cuda:
            return FrechetDistance.reference_moments(x, bins, J, table)
        lib, dev = _lib.load(), x.device
        ldx = max(x.stride(0), d) if n > 1 else d
        need = int(lib.mtrssm_feature_moments_workspace_bytes(n, d, J))
        if need < 0 or n * ldx >= 1 << 31:
            msg = f"feature moments: N {n}, D {d}, J {J}, ldx {ldx} are out of range (N * ldx < 2^31)"
            raise ValueError(msg)
        ws = _workspace(dev, need)
        _lib.check(_lib.TIMERS.call("mtrssm_feature_moments", lib.mtrssm_feature_moments, _lib.raw_ptr(x), ldx, _lib.index_ptr(bins.contiguous()), n, d,
                                    J, _lib.raw_ptr(table), ws.data_ptr(), ws.numel() * 8, _lib.stream_ptr(dev), flops=2.0 * n * d * (d + 1),
                                    nbytes=4.0 * n * (d + 1)), "mtrssm_feature_moments")
        return table


class FrechetTable(SumTable):
    """The accumulated moments of any number of Frechet steps in ONE float64 buffer ``[streams, 2 (real, generated), J, 1 + D + D * D]``
    (``block(stream, side)`` is what ``FrechetDistance.fold`` adds onto).  ``streams``: names; ``dims``: ``D``, shared by the streams;
    ``bins``: the bins' names (kept as ``bin_names``).  A step run with ``keep_states`` also leaves ``features`` (per stream ``(real
    [B * T, D], generated [B * S * T, D])``), ``bins`` = ``(real [B * T], generated [B * S * T])``, the rows' int32 bins, and ``states``
    here; otherwise they are None."""

    def __init__(self, streams: tuple[str, ...], dims: int, bins: tuple[str, ...], device: torch.device | str = "cpu") -> None:
        streams, bins = tuple(str(s) for s in streams), tuple(str(b) for b in bins)
        if isinstance(dims, (tuple, list)):
            if len(set(dims)) != 1:
                msg = f"the streams of a table share one D, got {dims!r}"
                raise ValueError(msg)
            dims = dims[0]
        dims = int(dims)
        if not streams or len(set(streams)) != len(streams) or not 1 <= dims <= MAX_DIM or not 1 <= len(bins) <= MAX_BINS:
            msg = f"need distinct streams, 1 <= D <= {MAX_DIM} and 1 .. {MAX_BINS} bins, got {streams!r}, D {dims} and {bins!r}"
            raise ValueError(msg)
        self.streams, self.dim, self.bin_names = streams, dims, bins
        self.buffer = torch.zeros(len(streams), len(SIDES), len(bins), cells(dims), dtype=torch.float64, device=device)
        self.features: dict[str, tuple[Tensor, Tensor]] | None = None
        self.bins: tuple[Tensor, Tensor] | None = None
        self.states = None

    def _key(self) -> tuple:
        return (self.streams, self.dim, self.bin_names)

    def matches(self, streams: tuple[str, ...], dim: int, bins: tuple[str, ...]) -> bool:
        return self._key() == (tuple(streams), int(dim), tuple(bins))

    def _sizes(self, other: SumTable) -> str:
        return f"{self._key()} and {other._key() if isinstance(other, FrechetTable) else type(other).__name__}"  # noqa: SLF001

    def add(self, other):  # noqa: ANN001, ANN201
        if not isinstance(other, FrechetTable) or other._key() != self._key():  # noqa: SLF001
            msg = f"tables of {self._sizes(other)} do not add"
            raise ValueError(msg)
        return super().add(other)

    def block(self, stream: int | str, side: int | str) -> Tensor:
        """``[J, 1 + D + D * D]``: a contiguous view of one stream's real (0) or generated (1) moments."""
        s = self.streams.index(stream) if isinstance(stream, str) else stream
        k = SIDES.index(side) if isinstance(side, str) else side
        return self.buffer[s, k]

    def state_dict(self) -> dict[str, object]:
        return {"buffer": self.buffer.detach().cpu().clone(), "streams": self.streams, "dim": self.dim, "bins": self.bin_names}

    def load_state_dict(self, state: dict[str, object]) -> None:
        key = (tuple(state["streams"]), int(state["dim"]), tuple(state["bins"]))
        if key != self._key() or tuple(state["buffer"].shape) != tuple(self.buffer.shape):
            msg = f"a saved table of {key} does not load into one of {self._key()}"
            raise ValueError(msg)
        self.buffer.copy_(state["buffer"])

    # -- the distance, on the host ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _gaussian(block: Tensor, d: int) -> tuple[Tensor, Tensor]:
        n = block[0]
        mu = block[1 : 1 + d] / n
        cov = block[1 + d :].reshape(d, d) / n - torch.outer(mu, mu)
        return mu, 0.5 * (cov + cov.t())

    @staticmethod
    def distance(real: Tensor, generated: Tensor, d: int) -> dict[str, float]:
        """The parts of the Frechet distance of two bins' moments (``[1 + D + D * D]`` float64 on the host)."""
        nan = float("nan")
        n_r, n_g = float(real[0]), float(generated[0])
        if min(n_r, n_g) < 2:  # noqa: PLR2004
            return {"fd": nan, "mean": nan, "cov": nan, "trace_ratio": nan, "n_real": n_r, "n_generated": n_g}
        (mu_r, cov_r), (mu_g, cov_g) = FrechetTable._gaussian(real, d), FrechetTable._gaussian(generated, d)
        w, q = torch.linalg.eigh(cov_r)
        root = (q * w.clamp_min(0.0).sqrt()) @ q.t()
        inner = root @ cov_g @ root
        lam = torch.linalg.eigvalsh(0.5 * (inner + inner.t())).clamp_min(0.0)
        tr_r, tr_g = float(torch.trace(cov_r)), float(torch.trace(cov_g))
        mean = float(((mu_r - mu_g) ** 2).sum())
        cov = tr_r + tr_g - 2.0 * float(lam.sqrt().sum())
        return {"fd": max(mean + cov, 0.0), "mean": mean, "cov": cov, "trace_ratio": tr_g / tr_r if tr_r > 0 else nan, "n_real": n_r,
                "n_generated": n_g}

    def compute(self) -> dict[str, dict[str, Tensor]]:
        """Per stream ``{fd, mean, cov, trace_ratio, n_real, n_generated}``, float64 ``[J]`` each on the host: one copy of the buffer,
        then ``distance`` per bin.  A bin with fewer than 2 rows on either side gives NaN."""
        host = self.buffer.detach().to("cpu")
        out: dict[str, dict[str, Tensor]] = {}
        for s, stream in enumerate(self.streams):
            per = [self.distance(host[s, 0, j], host[s, 1, j], self.dim) for j in range(len(self.bin_names))]
            out[stream] = {key: torch.tensor([p[key] for p in per], dtype=torch.float64) for key in per[0]}
        return out

    def scalars(self, prefix: str) -> dict[str, Tensor]:
        """``prefix/{stream}/{fd,mean,cov,trace_ratio,n}/{obs,h1,...}``, fp32 on the host (``n``: the real rows of the bin; the generated
        side has ``samples`` times as many)."""
        got = self.compute()
        return {f"{prefix}/{stream}/{part}/{name}": got[stream]["n_real" if part == "n" else part][j].to(torch.float32)
                for stream in self.streams for part in PARTS for j, name in enumerate(self.bin_names)}


__all__ = ["FrechetDistance", "FrechetTable", "bin_names", "cells"]
