"""A device-resident clip pool: the training data path.

The reference's loop draws every batch through audiotools' AudioDataset (scripts/train.py:440-475, `duration: 1.0` in
conf/base.yml:166): a random file, a random excerpt of it, re-drawn up to eight times until the excerpt's ITU-R BS.1770 loudness
exceeds -40 LUFS, so that silence is not trained on.  Here the whole corpus sits in device memory as one float32 arena (16 kHz mono is
64 kB/s) and a batch is drawn where it is used: the host draws clip numbers and offsets, one launch measures every candidate
(csrc/wv_loudness.hip), one more picks and copies.

    pool = ClipPool(clips, sample_rate=16000)            # or ClipPool.from_files(paths, 16000)
    x, info = pool.sample(64, duration=1.0, rng=0)       # x [64, 1, 16000] float32 on the device
    outs = trainer.fit(pool, steps=100, batch=64)

Loudness is this project's restatement of the published standard (waveverify_amd/loudness.py), and the accept rule -- the first try
strictly above the cutoff, else the LAST try -- is how audiotools' `salient_excerpt` is remembered to behave: both are this project's
rules, and parity with audiotools stays unpinned."""
from __future__ import annotations

from typing import Dict, Iterator, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from . import loudness as L


class ClipPool:
    """`clips`: 1-D float tensors or arrays, each one clip at `sample_rate`.  Immutable once built: one float32 arena on `device` plus
    the clips' int64 offsets and lengths.  len(pool) is the number of clips, pool.seconds their total duration."""

    def __init__(self, clips: Sequence, sample_rate: int = 16000, device="cuda"):
        arrays = []
        for i, c in enumerate(clips):
            a = c.detach().cpu().numpy() if torch.is_tensor(c) else np.asarray(c)
            if a.ndim != 1 or a.size == 0:
                raise ValueError(f"ClipPool: clip {i} must be 1-D and non-empty, got shape {tuple(a.shape)}")
            arrays.append(np.ascontiguousarray(a, dtype=np.float32))
        if not arrays:
            raise ValueError("ClipPool: no clips")
        L.sub_block(sample_rate)                                    # refuses a rate the gate cannot measure
        self._sample_rate = int(sample_rate)
        self._lengths = np.array([len(a) for a in arrays], np.int64)
        self._offsets = np.concatenate([[0], np.cumsum(self._lengths)[:-1]]).astype(np.int64)
        self._lengths.setflags(write=False)
        self._offsets.setflags(write=False)
        self._arena = torch.from_numpy(np.concatenate(arrays)).to(device)
        if not self._arena.is_cuda:
            raise RuntimeError("ClipPool: the pool lives on the GPU (there is no host route)")

    @classmethod
    def from_files(cls, paths: Sequence, sample_rate: int = 16000, device="cuda") -> "ClipPool":
        """Every file decoded, mixed down and resampled to `sample_rate` by utils.load_audio."""
        from .utils import load_audio
        return cls([load_audio(p, sample_rate)[0][0] for p in paths], sample_rate, device)

    sample_rate = property(lambda self: self._sample_rate)
    arena = property(lambda self: self._arena)
    offsets = property(lambda self: self._offsets)
    lengths = property(lambda self: self._lengths)

    def __len__(self) -> int:
        return len(self._lengths)

    @property
    def seconds(self) -> float:
        return float(self._lengths.sum()) / self._sample_rate

    def sample(self, batch: int, duration: float = 1.0, rng: Union[np.random.Generator, int, None] = None,
               loudness_cutoff: Optional[float] = -40.0, num_tries: int = 8) -> Tuple[torch.Tensor, Dict[str, np.ndarray]]:
        """-> (x [B, 1, T] float32 on the pool's device, info), T = round(duration * sample_rate).

        The draws, all on the host and in this order (loudness.draw): c = rng.integers(len(pool), size=B); u = rng.random((B, num_tries));
        offset[b, k] = floor(u[b, k] * (max(len_c - T, 0) + 1)); lens = min(len_c, T) (a clip shorter than T is zero-padded).  Then one
        wv_loudness over the B x num_tries candidates, one wv_pool_sample, and no other device work.  This project's accept rule: the
        FIRST try whose loudness is strictly above `loudness_cutoff`, else the LAST try (parity with audiotools unpinned, see the
        module's docstring).  loudness_cutoff=None takes try 0 and measures nothing.

        info: `clip`, `offset` (of the accepted try, in the clip), `tries_used` (accepted try + 1), `lufs` (of the accepted try; nan
        without a cutoff), all [B] on the host -- reading them back waits for the two launches."""
        from .metrics import loudness_windows
        B, tries, T = int(batch), int(num_tries), int(round(float(duration) * self._sample_rate))
        if B < 1 or tries < 1 or T < 1:
            raise ValueError(f"ClipPool.sample: batch {batch}, num_tries {num_tries} and duration {duration} must all be positive")
        rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        clip, offset, lens = L.draw(rng, self._lengths, B, T, tries)
        if loudness_cutoff is None:
            offset, tries = offset[:, :1], 1
        dev = self._arena.device
        starts = torch.from_numpy(np.ascontiguousarray(self._offsets[clip][:, None] + offset)).to(dev)
        lens_d = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(lens[:, None], (B, tries)).astype(np.int32))).to(dev)
        lufs = None
        if loudness_cutoff is not None:
            lufs, _, _ = loudness_windows(self._arena, starts.reshape(-1), lens_d.reshape(-1), T, self._sample_rate)
        x = torch.empty(B, 1, T, dtype=torch.float32, device=dev)
        choice = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().wv_pool_sample(self._arena.data_ptr(), starts.data_ptr(), lens_d.data_ptr(), _lib.ptr(lufs), B, tries, T,
                                              float(loudness_cutoff if loudness_cutoff is not None else 0.0), x.data_ptr(), choice.data_ptr(),
                                              _lib.stream(dev)), "wv_pool_sample")
        k = choice.cpu().numpy().astype(np.int64)
        rows = np.arange(B)
        chosen = lufs.cpu().numpy().reshape(B, tries)[rows, k] if lufs is not None else np.full(B, np.nan)
        return x, {"clip": clip, "offset": offset[rows, k], "tries_used": k + 1, "lufs": chosen}

    def batches(self, batch: int, duration: float = 1.0, seed: int = 0, **sample_kwargs) -> Iterator[torch.Tensor]:
        """An endless iterator of x, every batch drawn from the one generator seeded with `seed`."""
        rng = np.random.default_rng(seed)
        while True:
            yield self.sample(batch, duration, rng=rng, **sample_kwargs)[0]
