"""Byte input of the bf16 full-AlexNet engine, the parts that need no GPU: the C ABI's new symbols and their
null-argument errors, the knob, and the address plan of the row-band Conv1's byte loader."""
import ctypes as C

import pytest

from anx import _native as nat
from anx.utils.tuning import KNOBS, default_knob, knob_value

NEW = ("anx_full_run", "anx_full_set_input_norm", "anx_full_last_input")


def test_symbols_exported_and_declared():
    lib = nat.bf16()
    for name in NEW:
        assert name in nat._BF16_SIGS, name
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.argtypes == nat._BF16_SIGS[name][1] and fn.restype is nat._BF16_SIGS[name][0]


def test_abi_version_3():
    assert nat.lib().anx_abi_version() >= 3


def test_bf16_u8_knob():
    assert "bf16_u8" in KNOBS
    assert knob_value("bf16_u8", True) == 1 and knob_value("bf16_u8", False) == 0
    assert knob_value("bf16_u8", 1) == 1 and knob_value("bf16_u8", 0) == 0
    with pytest.raises(ValueError):
        knob_value("bf16_u8", 2)
    assert default_knob("bf16_u8") in (0, 1)


def test_null_engine_is_an_error_with_a_message():
    lib = nat.bf16()
    buf = C.create_string_buffer(32)
    three = (C.c_float * 3)(1.0, 1.0, 1.0)
    for name, args in (("anx_full_last_input", (None, buf, len(buf))),
                       ("anx_full_set_input_norm", (None, three, three)),
                       ("anx_full_run", (None, C.byref(nat.FullCallC(rows=1)), None)),  # floats
                       ("anx_full_run", (None, C.byref(nat.FullCallC(rows=1, u8=1)), None)),  # bytes
                       ("anx_full_run", (None, C.byref(nat.FullCallC(rows=1, mark=1)), None)),
                       ("anx_full_run", (None, C.byref(nat.FullCallC(rows=1, u8=1, mark=1)), None))):
        assert getattr(lib, name)(*args) != 0, name
        msg = nat.lib().anx_last_error().decode()
        assert name in msg and "no engine" in msg, (name, msg)


def test_full_run_refuses_a_null_call_and_a_wrong_size():
    """anx_full_run checks the call, then its size, then the engine: a null engine reaches "no engine" only with the
    size the library accepts, which is therefore ctypes' sizeof(FullCallC)."""
    lib, err = nat.bf16(), lambda: nat.lib().anx_last_error().decode()
    for engine in (None, C.c_void_p()):  # the size is looked at before the engine: a null engine changes nothing
        assert lib.anx_full_run(engine, None, None) != 0
        assert err().startswith("anx_full_run: ")
        short = nat.FullCallC(rows=1)
        short.size = C.sizeof(nat.FullCallC) - 8
        assert lib.anx_full_run(engine, C.byref(short), None) != 0
        assert err().startswith("anx_full_run: ") and "size" in err(), err()
    ok = nat.FullCallC(rows=1)
    assert ok.size == C.sizeof(nat.FullCallC)
    assert lib.anx_full_run(None, C.byref(ok), None) != 0
    assert "no engine" in err() and "size" not in err(), err()


# ---- the byte loader's address plan (conv1_bf16_ring.hip, "U8: the same plan in bytes"), mirrored from the kernel's
# comment: it documents the plan and checks its arithmetic; it cannot test the kernel.
ROW, ROWS, COLS = 681, 227, 57  # bytes per image row; image rows; polyphase columns
IMAGE = ROWS * ROW


def loads(wave, lane, pr):
    """The three dword loads of lane `lane` of wave `wave` for polyphase row `pr` of one image:
    [(byte offset, length)], [] where the lane loads nothing (its offset lies past the extent: zeros)."""
    row = 4 * pr + wave
    if pr >= COLS or row >= ROWS or lane >= COLS:
        return []
    b = row * ROW + 12 * lane
    return [(b, 4), (b + 4, 4), (b + (5 if lane == COLS - 1 else 8), 4)]


def used(wave, lane, pr):
    """The bytes of those loads the lane decodes: 12, or column 56's 9 (bytes 0-7 of the first two dwords and
    byte 8, the top byte of the third, which sits at +5)."""
    ld = loads(wave, lane, pr)
    if not ld:
        return []
    b = ld[0][0]
    if lane == COLS - 1:
        assert ld[2] == (b + 5, 4) and ld[2][0] + 3 == b + 8
        return list(range(b, b + 9))
    return list(range(b, b + 12))


def test_byte_loader_address_plan():
    seen = bytearray(IMAGE)
    for pr in range(COLS + 3):  # rows past the image: tiles reach polyphase row 59
        for wave in range(4):
            for lane in range(64):
                for off, n in loads(wave, lane, pr):
                    assert 0 <= off and off + n <= IMAGE  # the last image's last row: not a byte past the tensor
                    row = off // ROW
                    assert off + n <= (row + 1) * ROW  # nor past its own row
                for e in used(wave, lane, pr):
                    seen[e] += 1
    assert seen == bytearray([1]) * IMAGE  # every byte of rows 0-226 decoded exactly once
    # column 56's shifted load ends at the row's last byte; its plain position would reach 3 bytes past it
    last = loads(2, COLS - 1, 56)  # image row 226, the last
    assert last[2][0] + last[2][1] == IMAGE and last[0][0] + 8 + 4 == IMAGE + 3
    assert loads(3, 0, 56) == [] and loads(0, COLS, 0) == [] and loads(0, 0, COLS) == []  # row 227, lane 57, row 228+
