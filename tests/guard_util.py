"""One guarded arena for the memory tests of the PPO ABI (test_ppo_memory_gpu.py): a single int32
allocation filled with a canary, out of which named sub-buffers are handed, each 256-byte aligned
with guard words before it, after it and between it and its neighbours.  A store past a buffer's
end therefore lands in guard words inside the allocation, where check() finds it, instead of in
the allocator's slack or in a neighbour tensor.

The guard width is a condition, not a measurement: at least GUARD_ROWS rows of the buffer's own
row pitch and at least GUARD_MIN_WORDS words, on each side.  The kernels under test work in 16-,
32- and 64-row tiles, so the worst overrun a ragged tile could commit is below 64 rows.

Roles.  Every buffer has one, changeable between calls (set_role):
  "output"     the call may write it; only its guards are checked
  "input"      arm() snapshots it, check() wants it bit-identical to the snapshot
  "unwritten"  an output the call was not asked for: arm() fills it, check() wants the fill intact

Plain is the same interface over separate zero-initialised, unguarded allocations (the conditions
the kernels run under outside these tests), so one piece of test code drives both."""

import torch

CANARY = 0x7FC0BEEF  # a NaN no output holds (the guards of test_grid_gpu.py / test_observe_gpu.py)
FILL = 0x7FC12345    # another, for outputs a call must leave alone
GUARD_ROWS = 64
GUARD_MIN_WORDS = 256
ALIGN_WORDS = 64     # 256 bytes
ROLES = ("output", "input", "unwritten")


def guard_words(row_words):
    """Guard width of a buffer whose rows are row_words 32-bit words long."""
    return max(GUARD_MIN_WORDS, GUARD_ROWS * int(row_words))


def _up(x, a=ALIGN_WORDS):
    return -(-x // a) * a


class _Buf:
    def __init__(self, name, words, row_words, role):
        assert role in ROLES, role
        assert words >= 1 and row_words >= 1
        self.name, self.words, self.row_words, self.role = name, int(words), int(row_words), role
        self.guard = guard_words(row_words)
        self.start = None  # word offset of the buffer inside the arena, set by build()
        self.snap = None


class Arena:
    def __init__(self, device):
        self.device = torch.device(device)
        self.bufs = {}
        self.mem = None

    # ------------------------------------------------------------------ layout
    def add(self, name, words, row_words=1, role="output"):
        """Reserve `words` 32-bit words under `name` (before build())."""
        assert self.mem is None and name not in self.bufs, name
        self.bufs[name] = _Buf(name, words, row_words, role)
        return name

    def build(self):
        """Lay the buffers out and allocate: [guard | buf | guard | buf | ... | guard], a guard
        between neighbours as wide as the wider of the two asks for, every buffer 256-byte aligned
        whatever the allocation's own alignment."""
        assert self.mem is None and self.bufs
        order = list(self.bufs.values())
        pos, prev = 0, 0
        for b in order:
            pos = _up(pos + max(prev, b.guard))
            b.start = pos
            pos += b.words
            prev = b.guard
        total = pos + prev
        self.mem = torch.full((total + ALIGN_WORDS,), CANARY, dtype=torch.int32, device=self.device)
        shift = (-(self.mem.data_ptr() // 4)) % ALIGN_WORDS
        self.arena = self.mem[shift:shift + total]
        mask = torch.ones(total, dtype=torch.bool)
        for b in order:
            mask[b.start:b.start + b.words] = False
        self.guard_mask = mask.to(self.device)
        for b in order:
            assert self.ptr(b.name) % 256 == 0
            self.words(b.name).zero_()
        return self

    # ------------------------------------------------------------------ access
    def words(self, name):
        """The buffer as int32 words (a view of the arena)."""
        b = self.bufs[name]
        return self.arena[b.start:b.start + b.words]

    def f32(self, name):
        return self.words(name).view(torch.float32)

    def i64(self, name):
        return self.words(name).view(torch.int64)

    def u8(self, name):
        return self.words(name).view(torch.uint8)

    def ptr(self, name):
        return self.words(name).data_ptr()

    def names(self):
        return list(self.bufs)

    def set_role(self, role, *names):
        assert role in ROLES, role
        for n in names:
            self.bufs[n].role = role

    # ------------------------------------------------------------------ the check
    def arm(self):
        """Before a call: snapshot every input, fill every output that was not asked for."""
        for b in self.bufs.values():
            b.snap = None
            if b.role == "input":
                b.snap = self.words(b.name).clone()
            elif b.role == "unwritten":
                self.words(b.name).fill_(FILL)

    def _where(self, pos):
        """(name, offset) of the buffer nearest to arena word `pos` (a guard word): a negative
        offset lies before the buffer's first word, one >= its size past its last."""
        best = None
        for b in self.bufs.values():
            off = pos - b.start
            dist = -off if off < 0 else off - (b.words - 1)
            if best is None or dist < best[0]:
                best = (dist, b.name, off, b.words)
        return best[1:]

    def check(self, what=""):
        """After a call (the caller has synchronised): every guard word intact, every input
        bit-identical to arm()'s snapshot, every unwritten output still FILL."""
        bad = (self.arena != CANARY) & self.guard_mask
        if bool(bad.any()):
            pos = int(bad.nonzero()[0])
            name, off, words = self._where(pos)
            side = "before" if off < 0 else "past the end of"
            raise AssertionError(
                f"{what}: guard word written {side} '{name}' at word offset {off} of its {words}"
                f" ({int(bad.sum())} guard words changed; value 0x{int(self.arena[pos]) & 0xFFFFFFFF:08X})")
        for b in self.bufs.values():
            w = self.words(b.name)
            if b.role == "input":
                assert b.snap is not None, f"{what}: input '{b.name}' was not armed"
                diff = w != b.snap
                if bool(diff.any()):
                    off = int(diff.nonzero()[0])
                    raise AssertionError(
                        f"{what}: input '{b.name}' changed at word offset {off} of its {b.words}"
                        f" (0x{int(b.snap[off]) & 0xFFFFFFFF:08X} -> 0x{int(w[off]) & 0xFFFFFFFF:08X};"
                        f" {int(diff.sum())} words differ)")
            elif b.role == "unwritten":
                diff = w != FILL
                if bool(diff.any()):
                    off = int(diff.nonzero()[0])
                    raise AssertionError(
                        f"{what}: output '{b.name}', which the call was not asked for, was written"
                        f" at word offset {off} of its {b.words} ({int(diff.sum())} words)")


class Plain:
    """Arena's interface over separate zero-initialised allocations without guards."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.sizes = {}
        self.t = None

    def add(self, name, words, row_words=1, role="output"):
        assert self.t is None and name not in self.sizes, name
        self.sizes[name] = int(words)
        return name

    def build(self):
        self.t = {n: torch.zeros(w, dtype=torch.int32, device=self.device)
                  for n, w in self.sizes.items()}
        return self

    def words(self, name):
        return self.t[name]

    def f32(self, name):
        return self.t[name].view(torch.float32)

    def i64(self, name):
        return self.t[name].view(torch.int64)

    def u8(self, name):
        return self.t[name].view(torch.uint8)

    def ptr(self, name):
        return self.t[name].data_ptr()

    def names(self):
        return list(self.sizes)

    def set_role(self, role, *names):
        pass

    def arm(self):
        pass

    def check(self, what=""):
        pass
