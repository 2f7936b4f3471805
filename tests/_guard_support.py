"""Shared test support for tests/test_image_guards.py: operands inside poisoned guards, and the checks that see where a query read and
wrote, not only what it computed.

Every operand of a call — input, output, in/out, scratch — is the middle of one flat buffer of 4-byte words, ``guard + words + guard``
with ``guard = max(4096, words)``: a store one tile row past the end, a scratch overrun by a few words or a load from beyond the last
row lands inside that buffer, where it neither faults nor goes unseen.  The harness DETECTS stray accesses; no case may place an
operand so that an overrun would leave its allocation.

    guarded(words, poison)        (whole, view): the buffer and its middle, a numpy array or a CUDA tensor
    Case                          the operands of one call, in one form ("numpy" or "cuda") and one poison round
        compact / field / temp    an operand whose payload is compact, a strided field of records, or scratch
        finish                    after the call: downloads every buffer
    check_written(case, want)     guards and record filler untouched, inputs unchanged, no output element left unwritten
    run_poisoned(build, call, want, form)
                                  the case three times, with three contents in every guard, every record filler, every scratch and
                                  the pre-fill of every pure output; the three results bit-identical to each other and to ``want``

The poisons of a float plane are 0x5A5A5A5A (a large finite value, 1.5e16), -5.0 and a quiet NaN — a NaN alone would be masked by the
queries that skip non-finite pixels by definition; those of an integer plane a word that reads as valid and in range (1), zero and
0xFFFFFFFF.  A result that moves with the poison was computed from words outside the operands, or from scratch or output words read
before they were written; the failure names the operands whose poison moved it (found by varying one operand at a time, after the
failure only).  Imports without a GPU: torch is loaded by the "cuda" form alone.
"""
import numpy as np

F32, U32 = np.float32, np.uint32
SENTINEL = 0x5A5A5A5A
FLOAT_POISONS = (SENTINEL, 0xC0A00000, 0x7FC00000)  # 1.5e16, -5.0, a quiet NaN
INT_POISONS = (1, 0, 0xFFFFFFFF)
ROUNDS = 3
MIN_GUARD = 4096
ROLES = ("in", "out", "inout", "temp")


def poison(kind, k):
    return (FLOAT_POISONS if kind == "f" else INT_POISONS)[k]


def guard_words(words, align_words=8):
    g = max(MIN_GUARD, int(words))
    return (g + align_words - 1) // align_words * align_words


def guarded(words, poison, align_words=8, form="numpy"):
    """(whole, view): one flat buffer of guard + words + guard 4-byte words, every one ``poison``, and its contiguous middle; the
    guard is max(4096, words) rounded up to ``align_words``, so the middle of a 32-byte aligned buffer is 32-byte aligned.  A uint32
    numpy array, or (form "cuda") an int32 CUDA tensor."""
    words, g = int(words), guard_words(words, align_words)
    total = 2 * g + words
    if form == "cuda":
        from _records import torch_device

        torch = torch_device()
        whole = torch.from_numpy(np.full(total, poison, dtype=U32).view(np.int32)).cuda()
    else:
        spare = np.full(total + align_words, poison, dtype=U32)  # numpy promises 16 bytes: start at the first 32-byte boundary
        skip = (-spare.ctypes.data // 4) % align_words
        whole = spare[skip:skip + total]
    return whole, whole[g:g + words]


def bits(a):
    return np.ascontiguousarray(a).view(U32).reshape(-1)


def same_bits(got, want):
    g, w = bits(got), bits(want)
    return g.shape == w.shape and bool((g == w).all())


def same_or_both_nan(got, want):
    """for float32 planes: bit-identical, or both NaN (the sign and payload of a NaN that went through arithmetic differ by machine)"""
    g, w = bits(got), bits(want)
    return g.shape == w.shape and bool(((g == w) | (np.isnan(g.view(F32)) & np.isnan(w.view(F32)))).all())


class Operand:
    """One guarded operand.  ``view`` is what the call is given; ``whole`` the buffer around it; ``guard`` and ``words`` its layout in
    words; ``payload`` marks the words (bytes, for byte planes) of the buffer that belong to the operand."""

    def __init__(self, case, name, role, kind, shape, dtype, record, record_words, at, width, data):
        assert role in ROLES and name not in case.operands, name
        self.name, self.role, self.kind, self.form = name, role, kind, case.form
        self.shape, self.dtype, self.record, self.record_words, self.at, self.width = tuple(shape), np.dtype(dtype), record, record_words, at, width
        k_guard, k_filler, k_temp, k_prefill = (case.round_of(name, g) for g in ("guards", "filler", "temp", "prefill"))
        if record_words:  # a field of `width` words at word `at` of records of `record_words` words
            self.nbytes = int(np.prod(self.shape[:len(self.shape) - (width > 1)], dtype=np.int64)) * record_words * 4
        else:
            self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.words = (self.nbytes + 3) // 4
        self.guard = guard_words(self.words)
        host = np.full(2 * self.guard + self.words, poison(kind, k_guard), dtype=U32)
        middle = host[self.guard:self.guard + self.words]
        self.prefill = poison(kind, k_temp if role == "temp" else k_prefill)
        middle[:] = poison(kind, k_filler) if record_words or data is not None else self.prefill
        self.payload = np.zeros(host.size * 4, dtype=bool)
        self._np_view(self.payload.view(np.uint8), as_bytes=True)[...] = 1
        if data is not None:
            data = np.asarray(data)
            assert data.dtype.itemsize == self.dtype.itemsize and data.size == int(np.prod(self.shape, dtype=np.int64)), name
            self._np_view(host.view(np.uint8))[...] = data.view(self.dtype).reshape(self.shape)
        elif record_words:
            self._np_view(host.view(np.uint8))[...] = np.array(self.prefill, dtype=U32).view(self.dtype)
        self.before = host.view(np.uint8).copy()
        self.after = None
        if self.form == "cuda":
            from _records import torch_device

            torch = torch_device()
            self.whole = torch.from_numpy(host.view(np.int32)).cuda()
            self.view = self._torch_view(torch)
        else:
            self.whole, _ = guarded(self.words, 0)
            self.whole[:] = host
            self.view = self._np_view(self.whole.view(np.uint8))

    def _np_view(self, buffer, as_bytes=False):
        """the operand's view of a host image of the buffer (uint8); ``as_bytes``: of a byte mask with one entry per byte"""
        middle = buffer[self.guard * 4:self.guard * 4 + self.words * 4]
        if as_bytes:  # the same slicing, on bytes: one more trailing dimension of itemsize
            if self.record_words:
                records = middle.reshape(-1, self.record_words, 4)
                return records[:, self.at:self.at + self.width]
            return middle[:self.nbytes]
        if self.record_words:
            records = middle.view(self.dtype).reshape(self.shape[:len(self.shape) - (self.width > 1)] + (self.record_words,))
            return records[..., self.at:self.at + self.width] if self.width > 1 else records[..., self.at]
        return middle[:self.nbytes].view(self.dtype).reshape(self.shape)

    def _torch_view(self, torch):
        middle = self.whole[self.guard:self.guard + self.words]
        if self.record is not None:  # the device form of a record array: (n, words) of the record's device dtype
            return middle.view(getattr(torch, self.record[2])).view(-1, self.record[3])
        dtype = {"float32": torch.float32, "uint32": torch.int32, "int32": torch.int32, "uint8": torch.uint8}[self.dtype.name]
        if self.record_words:
            records = middle.view(dtype).view(self.shape[:len(self.shape) - (self.width > 1)] + (self.record_words,))
            return records[..., self.at:self.at + self.width] if self.width > 1 else records[..., self.at]
        return middle.view(dtype)[:self.nbytes // self.dtype.itemsize].view(self.shape)

    def download(self):
        if self.form == "cuda":
            self.after = self.whole.cpu().numpy().view(np.uint8).copy()
        else:
            self.after = self.whole.view(np.uint8).copy()

    def got(self):
        """the payload after the call, as the numpy form holds it (a copy)"""
        return np.array(self._np_view(self.after))

    def given(self):
        """the payload before the call (a copy)"""
        return np.array(self._np_view(self.before))


class Case:
    """The guarded operands of one call.  ``form``: "numpy" or "cuda"; ``k``: the poison round of every operand; ``only``: (operand
    name, round) — that operand alone takes that round, the others round 0 (the follow-up that finds whose poison moved a result)."""

    def __init__(self, form="numpy", k=0, only=None):
        assert form in ("numpy", "cuda")
        self.form, self.k, self.only, self.operands = form, k, only, {}

    def round_of(self, name, group):
        if self.only is not None:
            return self.only[1] if name == self.only[0] else 0
        return self.k

    def compact(self, name, role, data=None, shape=None, dtype=F32, kind=None, record=None):
        """a compact operand: ``data`` (inputs and in/out operands), or ``shape`` and ``dtype`` of a pure output.  ``record``: the
        (label, numpy dtype, device dtype, words) of _forms — the numpy form is an array of that dtype, the device form (n, words)"""
        if data is not None:
            data = np.asarray(data)
            shape, dtype = data.shape, data.dtype
        if record is not None:
            dtype = record[1]
        dtype = np.dtype(dtype)
        kind = kind or ("i" if dtype.kind in "iu" else "f")
        return self._add(Operand(self, name, role, kind, shape, dtype, record, 0, 0, 0, data))

    def field(self, name, role, record_words, at, data=None, shape=None, dtype=F32, kind=None, width=1):
        """an operand the query takes as a strided view: the field of ``width`` words at word ``at`` of records of ``record_words``
        words; ``shape`` (or ``data``'s) is the pixels' shape, followed by ``width`` when that is more than one"""
        if data is not None:
            data = np.asarray(data)
            shape, dtype = data.shape, data.dtype
        dtype = np.dtype(dtype)
        kind = kind or ("i" if dtype.kind in "iu" else "f")
        assert dtype.itemsize == 4 and at + width <= record_words and (width == 1 or shape[-1] == width)
        return self._add(Operand(self, name, role, kind, shape, dtype, None, record_words, at, width, data))

    def temp(self, name, words, dtype=F32):
        """scratch of exactly ``words`` 4-byte words (``dtype`` uint8: the same bytes as a byte tensor)"""
        dtype = np.dtype(dtype)
        return self._add(Operand(self, name, "temp", "f", (int(words) * 4 // dtype.itemsize,), dtype, None, 0, 0, 0, None))

    def _add(self, op):
        self.operands[op.name] = op
        return op.view

    def __getitem__(self, name):
        return self.operands[name]

    def finish(self):
        if self.form == "cuda":
            from _records import torch_device

            torch_device().cuda.synchronize()
        for op in self.operands.values():
            op.download()

    def results(self):
        return {name: op.got() for name, op in self.operands.items() if op.role in ("out", "inout")}


def _where(op, byte):
    word = int(byte) // 4
    if word < op.guard:
        return f"{op.guard - word} words before its first"
    if word >= op.guard + op.words:
        return f"{word - op.guard - op.words + 1} words past its last"
    return f"at word {word - op.guard}, between the fields of its records"


def check_written(case, want=None):
    """After the call (``case.finish()`` is run here if it was not).  Asserts, naming the operand:
      - the guards of every operand still hold their poison, and so do the words of its records that are not its field;
      - every input holds what it held, over the whole buffer;
      - no word of a pure output still holds the pre-fill, unless ``want[name]`` says that is its value."""
    if any(op.after is None for op in case.operands.values()):
        case.finish()
    for op in case.operands.values():
        changed = op.after != op.before
        outside = changed & ~op.payload
        if outside.any():
            first = int(np.flatnonzero(outside)[0])
            what = "input" if op.role == "in" else {"out": "output", "inout": "in/out operand", "temp": "scratch"}[op.role]
            raise AssertionError(f"{what} '{op.name}' ({case.form}): {int(outside.sum() + 3) // 4} words outside it were written, the first "
                                 f"{_where(op, first)}")
        if op.role == "in" and changed.any():
            first = int(np.flatnonzero(changed)[0])
            raise AssertionError(f"input '{op.name}' ({case.form}): the call modified it, first at word {first // 4 - op.guard}")
        if op.role == "out":
            got = bits(op.got())
            still = got == U32(op.prefill)
            if want is not None and op.name in want:
                expect = bits(want[op.name])
                assert expect.shape == got.shape, (op.name, expect.shape, got.shape)
                still &= expect != U32(op.prefill)
            if still.any():
                raise AssertionError(f"output '{op.name}' ({case.form}): {int(still.sum())} words were left unwritten (they hold the pre-fill "
                                     f"{op.prefill:#x}), the first at word {int(np.flatnonzero(still)[0])}")


def _run(build, call, want, form, k=0, only=None):
    case = Case(form, k, only)
    ops = build(case)
    call(ops)
    case.finish()
    return case


def run_poisoned(build, call, want, form="numpy", same=None):
    """``build(case)`` adds the operands to a Case and returns what ``call`` takes; ``want``: {operand name: expected array} for every
    output and in/out operand; ``same``: {operand name: comparison}, ``same_bits`` where not given.  Runs the three rounds, each through
    check_written, and holds every result to ``want`` — so the three are equal to each other as well."""
    same = same or {}
    for k in range(ROUNDS):
        case = _run(build, call, want, form, k)
        check_written(case, want)
        got = case.results()
        assert set(got) == set(want), (sorted(got), sorted(want))
        for name in got:
            if (same.get(name) or same_bits)(got[name], want[name]):
                continue
            # which operand's poison moved it: one operand at a time at this round, the others at round 0
            base = _run(build, call, want, form, 0).results()[name]
            if k == 0 or not same_bits(base, got[name]):
                movers = []
                for other in case.operands.values():
                    alone = _run(build, call, want, form, 0, (other.name, k or 1)).results()[name]
                    if not same_bits(alone, base):
                        role = {"in": "the guards or record filler of input", "out": "the pre-fill or guards of output",
                                "inout": "the guards of in/out operand", "temp": "the contents of scratch"}[other.role]
                        movers.append(f"{role} '{other.name}'")
                if movers:
                    raise AssertionError(f"'{name}' ({form}) moves with the poison (round {k}) of " + ", ".join(movers) +
                                         ": the call read outside its operands, or read scratch or output before writing it")
            g, w = bits(got[name]), bits(want[name])
            bad = np.flatnonzero(g != w) if g.shape == w.shape else np.array([0])
            raise AssertionError(f"'{name}' ({form}, poison round {k}) differs from the CPU definition in {bad.size} words, the first at "
                                 f"word {int(bad[0])}; it does not move with any single operand's poison")
    return got
