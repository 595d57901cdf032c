"""guard_util.Arena on CPU tensors: what it must refuse, and that it names the buffer and the
offset.  (The GPU memory tests of the PPO ABI, test_ppo_memory_gpu.py, stand on this helper.)"""

import pytest
import torch

from guard_util import (ALIGN_WORDS, CANARY, FILL, GUARD_MIN_WORDS, GUARD_ROWS, Arena, Plain,
                        guard_words)

# name, words, row pitch in words, role: pitches on both sides of the 256-word floor, sizes that
# are no multiple of 64 words, a one-word buffer, and neighbours whose guards differ
SPEC = (("states", 23 * 60, 60, "input"), ("idx", 2 * 17, 2, "input"), ("value", 17, 1, "output"),
        ("grads", 1001, 1, "output"), ("logp", 17, 1, "unwritten"), ("one", 1, 1, "input"),
        ("workspace", 5000, 1024, "output"), ("tail", 65, 3, "unwritten"))


def _arena():
    a = Arena("cpu")
    for name, words, row, role in SPEC:
        a.add(name, words, row, role)
    a.build()
    g = torch.Generator().manual_seed(0)
    for name, words, _, role in SPEC:
        if role != "unwritten":
            a.words(name).copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, (words,), generator=g,
                                              dtype=torch.int64).to(torch.int32))
    a.arm()
    return a


def _guards(a, name):
    """Arena offsets of the first and last guard word of buffer `name`: its own guard width
    before its first word and past its last."""
    b = a.bufs[name]
    return b.start - b.guard, b.start + b.words + b.guard - 1


def test_guard_width_is_the_stated_condition():
    assert guard_words(1) == GUARD_MIN_WORDS == 256 and GUARD_ROWS == 64
    assert guard_words(4) == 256 and guard_words(5) == 320 and guard_words(1024) == 65536


def test_layout_alignment_and_guards_between_neighbours():
    a = _arena()
    order = [a.bufs[n] for n, *_ in SPEC]
    assert order[0].start >= order[0].guard
    for b in order:
        assert b.guard == max(256, 64 * b.row_words)
        assert a.ptr(b.name) % 256 == 0 and b.start % ALIGN_WORDS == 0
        lo, hi = _guards(a, b.name)
        assert lo >= 0 and hi < a.arena.numel()
        # the buffer's whole guard width on either side is guard words: no other buffer in it
        assert bool(a.guard_mask[lo:b.start].all())
        assert bool(a.guard_mask[b.start + b.words:hi + 1].all())
        assert not bool(a.guard_mask[b.start:b.start + b.words].any())
        assert bool((a.arena[lo:b.start] == CANARY).all())
    for p, q in zip(order, order[1:]):
        assert q.start - (p.start + p.words) >= max(p.guard, q.guard)
    assert a.arena.numel() - (order[-1].start + order[-1].words) >= order[-1].guard


def test_untouched_arena_passes_and_outputs_may_change():
    a = _arena()
    a.check("untouched")
    a.words("value").fill_(7)
    a.words("grads")[-1] = 1
    a.words("workspace").fill_(-1)
    a.check("outputs written in full")


@pytest.mark.parametrize("name", [s[0] for s in SPEC])
@pytest.mark.parametrize("side", ["first", "last"])
def test_one_word_into_a_guard_is_refused(name, side):
    a = _arena()
    lo, hi = _guards(a, name)
    a.arena[lo if side == "first" else hi] = 0
    with pytest.raises(AssertionError, match="guard word written"):
        a.check("probe")


@pytest.mark.parametrize("name", [s[0] for s in SPEC])
def test_guard_report_names_the_buffer_and_the_offset(name):
    b = _arena().bufs[name]
    for pos, off, side in ((b.start - 1, -1, "before"),
                           (b.start + b.words, b.words, "past the end of")):
        a = _arena()
        a.arena[pos] = 0x3F800000
        with pytest.raises(AssertionError) as e:
            a.check("probe")
        msg = str(e.value)
        assert f"{side} '{name}' at word offset {off} of its {b.words}" in msg, msg
        assert "0x3F800000" in msg and msg.startswith("probe")


@pytest.mark.parametrize("name", [s[0] for s in SPEC if s[3] == "input"])
@pytest.mark.parametrize("where", ["first", "last"])
def test_one_bit_of_an_input_is_refused(name, where):
    a = _arena()
    w = a.words(name)
    off = 0 if where == "first" else w.numel() - 1
    w[off] ^= 1
    with pytest.raises(AssertionError) as e:
        a.check("probe")
    assert f"input '{name}' changed at word offset {off} of its {w.numel()}" in str(e.value)


def test_sign_bit_of_an_input_is_refused():
    """-0.0 == 0.0 as floats; the comparison is on the words."""
    a = _arena()
    a.f32("states")[5] = 0.0
    a.arm()
    a.f32("states")[5] = -0.0
    with pytest.raises(AssertionError, match="input 'states' changed at word offset 5"):
        a.check("probe")


@pytest.mark.parametrize("name", [s[0] for s in SPEC if s[3] == "unwritten"])
def test_an_output_not_asked_for_must_keep_its_fill(name):
    a = _arena()
    assert bool((a.words(name) == FILL).all())
    a.words(name)[a.words(name).numel() - 1] = 0
    with pytest.raises(AssertionError, match=f"output '{name}', which the call was not asked for"):
        a.check("probe")


def test_roles_change_between_calls():
    a = _arena()
    a.set_role("input", "grads")
    a.arm()
    a.check("armed")
    a.words("grads")[3] += 1
    with pytest.raises(AssertionError, match="input 'grads' changed at word offset 3"):
        a.check("probe")
    a.set_role("output", "grads", "states")
    a.arm()
    a.words("states")[0] += 1
    a.check("states is an output now")
    a.set_role("input", "value")  # an input registered after arm() has no snapshot
    with pytest.raises(AssertionError, match="input 'value' was not armed"):
        a.check("probe")


def test_typed_views_share_the_arena():
    a = _arena()
    a.set_role("output", "idx")
    a.i64("idx")[0] = 2 ** 40 + 3
    assert int(a.words("idx")[0]) == 3 and int(a.words("idx")[1]) == 2 ** 8
    assert a.u8("value").numel() == 4 * 17 and a.f32("value").data_ptr() == a.ptr("value")
    a.check("typed writes inside a buffer")


def test_plain_has_the_interface_and_zeros():
    p = Plain("cpu")
    for name, words, row, role in SPEC:
        p.add(name, words, row, role)
    p.build()
    p.arm()
    for name, words, _, _ in SPEC:
        assert p.words(name).numel() == words and not bool(p.words(name).any())
        assert p.f32(name).data_ptr() == p.ptr(name)
    p.set_role("input", "states")
    p.check("nothing to check")
    assert p.names() == [s[0] for s in SPEC]
