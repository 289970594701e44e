"""Guard bands and poisoned workspaces for kernel tests (a plain module: `from guard import ...`).

An Arena is one buffer laid out as [lead guard | tensor | tail guard].  The guards hold a recognisable bit pattern (a quiet NaN with
payload for floats), so a store past either end of the tensor, or a read that reaches past it, shows up: the store as a changed guard,
the read as a NaN in the output.  Three placements:

- guarded_input(array): the data in a NaN arena; afterwards the whole arena, data included, must be bitwise unchanged.
- guarded_output(shape): the tensor itself is filled with the pattern too; afterwards the guards are intact and no element of the
  tensor still holds the pattern (every promised element was written), or exactly a given set of elements does.
- poisoned_workspace(nbytes): exactly nbytes filled with 0xFF (NaN as f32 and as f16) between guards; repoison() refills it.

The guards are at least max(1 MiB, size of the tensor) long, at most 64 MiB, and a multiple of 256 bytes, so offset=0 puts the tensor
on a 256-byte boundary and offset=1 one element past it."""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

MiB = 1 << 20
GUARD_MIN, GUARD_MAX = MiB, 64 * MiB

# dtype -> (integer view dtype, guard pattern as that integer)
_BITS = {
    torch.float32: (torch.int32, 0x7FA5A5A5),
    torch.float16: (torch.int16, 0x7E5A),
    torch.int32: (torch.int32, 0x5A5AA5A5),
    torch.int64: (torch.int64, 0x5A5AA5A55A5AA5A5),
    torch.uint8: (torch.uint8, 0xA5),
}
POISON_BYTE = 0xFF


class GuardError(AssertionError):
    pass


def _first_last(idx: torch.Tensor):
    return int(idx.min()), int(idx.max())


class Arena:
    """[lead guard | tensor | tail guard] in one buffer; .t is the tensor as a shaped view."""

    def __init__(self, shape, dtype=torch.float32, device="cuda", name="tensor", offset: int = 0, fill: str = "pattern"):
        if dtype not in _BITS:
            raise ValueError(f"no guard pattern for {dtype}")
        self.name, self.dtype, self.shape = name, dtype, tuple(int(s) for s in shape)
        self.ibits, self.pattern = _BITS[dtype]
        esz = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(self.shape, dtype=np.int64)) if self.shape else 1
        gbytes = min(max(GUARD_MIN, n * esz), GUARD_MAX)
        gbytes = -(-gbytes // 256) * 256
        self.g = gbytes // esz                         # guard length in elements (plus `offset` more in front)
        self.n, self.offset = n, int(offset)
        self.lo = self.g + self.offset                 # index of the tensor's first element in the buffer
        self.buf = torch.empty(self.lo + n + self.g, dtype=dtype, device=device)
        self._ibuf().fill_(self.pattern)
        if fill == "poison":
            self.tflat.view(torch.uint8).fill_(POISON_BYTE)
        self._snap: Optional[torch.Tensor] = None      # whole-arena snapshot for inputs
        self.unwritten_ok: Optional[torch.Tensor] = None

    def _ibuf(self) -> torch.Tensor:
        return self.buf.view(self.ibits)

    @property
    def tflat(self) -> torch.Tensor:
        return self.buf[self.lo: self.lo + self.n]

    @property
    def t(self) -> torch.Tensor:
        return self.tflat.view(self.shape)

    def repoison(self) -> None:
        self.tflat.view(torch.uint8).fill_(POISON_BYTE)

    def refill_pattern(self) -> None:
        self.tflat.view(self.ibits).fill_(self.pattern)

    # ------------------------------------------------------------------------------------------------ checks
    def guard_report(self) -> List[str]:
        ib = self._ibuf()
        out = []
        lead = (ib[: self.lo] != self.pattern).nonzero().flatten()
        if lead.numel():
            a, b = _first_last(lead)
            out.append(f"{self.name}: lead guard: {lead.numel()} element(s) changed, nearest at offset {b - self.lo} "
                       f"from the tensor's start (farthest {a - self.lo})")
        tail = (ib[self.lo + self.n:] != self.pattern).nonzero().flatten()
        if tail.numel():
            a, b = _first_last(tail)
            out.append(f"{self.name}: tail guard: {tail.numel()} element(s) changed, first at offset +{a} past the tensor's end "
                       f"(farthest +{b})")
        return out

    def check(self) -> None:
        msgs = self.guard_report()
        if msgs:
            raise GuardError("; ".join(msgs))


class GuardedInput(Arena):
    def __init__(self, array, device="cuda", name="input", offset: int = 0):
        a = array.detach() if isinstance(array, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(array))
        super().__init__(tuple(a.shape), a.dtype, device, name, offset)
        self.tflat.copy_(a.reshape(-1).to(device))
        self._snap = self.buf.clone()

    def check(self) -> None:
        msgs = self.guard_report()
        d = (self._ibuf()[self.lo: self.lo + self.n] != self._snap.view(self.ibits)[self.lo: self.lo + self.n]).nonzero().flatten()
        if d.numel():
            a, _ = _first_last(d)
            msgs.append(f"{self.name}: data: {d.numel()} element(s) of the input changed, first at offset {a}")
        if msgs:
            raise GuardError("; ".join(msgs))


class GuardedOutput(Arena):
    def __init__(self, shape, dtype=torch.float32, device="cuda", name="output", offset: int = 0):
        super().__init__(shape, dtype, device, name, offset)

    def unwritten(self) -> torch.Tensor:
        """Boolean mask (tensor-shaped) of the elements that still hold the pattern."""
        return (self.t.view(self.ibits) == self.pattern)

    def check(self, expect_unwritten: Optional[torch.Tensor] = None) -> None:
        """Guards intact and every element written; with expect_unwritten (bool mask, tensor-shaped) exactly those elements not."""
        msgs = self.guard_report()
        left = self.unwritten()
        want = torch.zeros_like(left) if expect_unwritten is None else expect_unwritten.to(left.device, torch.bool).reshape(left.shape)
        bad = (left != want).flatten().nonzero().flatten()
        if bad.numel():
            a, _ = _first_last(bad)
            n_left = int((left & ~want).sum())
            n_over = int((~left & want).sum())
            msgs.append(f"{self.name}: {n_left} element(s) left unwritten, {n_over} written that must not be; first at offset {a}")
        if msgs:
            raise GuardError("; ".join(msgs))


class PoisonedWorkspace(Arena):
    def __init__(self, nbytes: int, device="cuda", name="workspace"):
        super().__init__((int(nbytes),), torch.uint8, device, name, 0, fill="poison")


def guarded_input(array, device="cuda", name="input", offset: int = 0) -> GuardedInput:
    return GuardedInput(array, device, name, offset)


def guarded_output(shape, dtype=torch.float32, device="cuda", name="output", offset: int = 0) -> GuardedOutput:
    return GuardedOutput(shape, dtype, device, name, offset)


def poisoned_workspace(nbytes: int, device="cuda", name="workspace") -> PoisonedWorkspace:
    return PoisonedWorkspace(nbytes, device, name)


class Guards:
    """A set of arenas checked together: g.input(...), g.output(...), g.workspace(...), then g.check()."""

    def __init__(self, device="cuda", offset: int = 0):
        self.device, self.offset = device, offset
        self.arenas: List[Arena] = []

    def _add(self, a):
        self.arenas.append(a)
        return a

    def input(self, array, name="input", offset: Optional[int] = None) -> GuardedInput:
        return self._add(GuardedInput(array, self.device, name, self.offset if offset is None else offset))

    def output(self, shape, dtype=torch.float32, name="output", offset: Optional[int] = None) -> GuardedOutput:
        return self._add(GuardedOutput(shape, dtype, self.device, name, self.offset if offset is None else offset))

    def workspace(self, nbytes: int, name="workspace") -> PoisonedWorkspace:
        return self._add(PoisonedWorkspace(nbytes, self.device, name))

    def repoison(self) -> None:
        for a in self.arenas:
            if isinstance(a, PoisonedWorkspace):
                a.repoison()
            elif isinstance(a, GuardedOutput):
                a.refill_pattern()

    def check(self) -> None:
        if str(self.device).startswith("cuda"):
            torch.cuda.synchronize()
        msgs = []
        for a in self.arenas:
            try:
                a.check()
            except GuardError as e:
                msgs.append(str(e))
        if msgs:
            raise GuardError("\n".join(msgs))
