"""CPU: the value kernel's spec, key and caches (sail_jit.cpp, sail_capi.cpp). A value kernel is the scene's flat-form
run-time kernel with the decoded rows and the texParams table compiled in as 32-bit words; a context asks for it once
its rows have stood still for SAIL_DEBUG_JIT_VALUES_AFTER samples. Here: keys compare words (not floats), the source
prefix carries the words, the object compiles with hipRTC without a device, the user's cache keeps a bounded number
of value objects and never deletes a types kernel's, and the settle rule."""
import os
import re
import struct

import numpy as np

from sail_amd import capi


def _c1(fixtures):
    sc = dict(fixtures["scenes"]["C1"])
    sc["objects"] = list(sc["objects"])
    sc["texparams"] = list(sc["texparams"])
    return sc


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _set_f32(values, i, u):
    """values with element i replaced by the f32 of bit pattern u (NaN payloads survive: the list goes through numpy)"""
    a = np.asarray(values, np.float32).copy()
    a.view(np.uint32)[i] = u
    return a


def _words(defs, name):
    m = re.search(r"#define %s (.*)" % name, defs)
    assert m, defs[:400]
    return [int(w.rstrip("u"), 16) for w in m.group(1).split(", ")]


def _sphere_row(sc):
    rows = np.asarray(sc["objects"], np.float32).reshape(sc["n"], 18)
    return int(np.flatnonzero(rows[:, 0] == 2.0)[0])  # SAIL_SPHERE


def test_equal_rows_give_an_equal_key_and_the_prefix_carries_words(fixtures):
    sc = _c1(fixtures)
    k1, d1 = capi.jit_value_key(sc)
    k2, d2 = capi.jit_value_key(_c1(fixtures))
    assert k1 is not None and k1 == k2 and d1 == d2
    assert "#define SAIL_JIT_ROWVALS 1" in d1 and "#define SAIL_JIT_TPN %d\n" % sc["tn"] in d1
    rows, tp = _words(d1, "SAIL_JIT_ROW_WORDS"), _words(d1, "SAIL_JIT_TP_WORDS")
    assert len(rows) == sc["n"] * 32 and len(tp) == sc["tn"] * 16
    # the texParams words are the table's own bits; each row's first word is its shape id
    assert tp == np.asarray(sc["texparams"], np.float32).view(np.uint32).tolist()
    types = np.asarray(sc["objects"], np.float32).reshape(sc["n"], 18)[:, 0].astype(int).tolist()
    assert [rows[i * 32] for i in range(sc["n"])] == types
    # the sphere's centre and radius are in its row as the floats the scene gave
    s = _sphere_row(sc)
    obj = np.asarray(sc["objects"], np.float32).reshape(sc["n"], 18)[s]
    assert rows[s * 32 + 8:s * 32 + 12] == obj[1:5].view(np.uint32).tolist()
    # the text after the words is the types kernel's prefix: no float literal anywhere
    assert re.search(r"\d\.\d", d1) is None


def test_one_changed_word_gives_another_key(fixtures):
    base = _c1(fixtures)
    k0, _ = capi.jit_value_key(base)
    s = _sphere_row(base)
    keys = {"base": k0}

    moved = _c1(fixtures)
    moved["objects"] = _set_f32(moved["objects"], s * 18 + 1, _bits(float(np.float32(moved["objects"][s * 18 + 1]) + np.float32(0.25))))
    keys["moved bound"] = capi.jit_value_key(moved)[0]

    # +0 -> -0 and two NaN payloads in the sphere's emission (equal as floats, or unordered: different words)
    for name, u in (("+0", 0x00000000), ("-0", 0x80000000), ("nan a", 0x7fc00000), ("nan b", 0x7fc00001)):
        sc = _c1(fixtures)
        sc["objects"] = _set_f32(sc["objects"], s * 18 + 8, u)
        keys[name] = capi.jit_value_key(sc)[0]
        assert _words(capi.jit_value_key(sc)[1], "SAIL_JIT_ROW_WORDS")[s * 32 + 4] == u, name

    tpw = _c1(fixtures)
    tpw["texparams"] = _set_f32(tpw["texparams"], 1, _bits(0.6999999))
    keys["texParams word"] = capi.jit_value_key(tpw)[0]

    swapped = _c1(fixtures)
    rows = np.asarray(swapped["objects"], np.float32).reshape(swapped["n"], 18)[::-1].copy()
    swapped["objects"] = rows.reshape(-1)
    keys["swapped rows"] = capi.jit_value_key(swapped)[0]

    assert all(k is not None for k in keys.values()), keys
    assert keys.pop("+0") == k0  # the sphere's emission is +0 already: the same words, the same kernel
    assert len(set(keys.values())) == len(keys), keys


def test_scenes_without_a_value_kernel(fixtures):
    # the pre-cull form (64 rows) and the room form (LDS table copies) keep their types-only kernels
    for name in ("C4", "C3"):
        assert capi.jit_value_key(fixtures["scenes"][name]) == (None, ""), name


def test_settle_rule():
    assert not capi.plan_settle(0, 256) and not capi.plan_settle(255, 256)
    assert capi.plan_settle(256, 256) and capi.plan_settle(10**12, 256)
    assert capi.plan_settle(0, 0) and capi.plan_settle(5, 0)   # 0: at once
    for n in (0, 1, 256, 2**40):                                # negative: never
        assert not capi.plan_settle(n, -1) and not capi.plan_settle(n, -2**31)


def test_value_object_compiles_and_the_user_cache_is_capped(fixtures, tmp_path):
    """One hipRTC compile of a value kernel pair without a device (C1 with its sphere moved: no cache has it), into a user
    cache whose value directory (<dir>-values, beside the types kernels' <dir>) already holds the cap's worth of objects:
    the oldest value objects go, one for each object written, and no types kernel's object is touched."""
    sc = _c1(fixtures)
    s = _sphere_row(sc)
    sc["objects"] = _set_f32(sc["objects"], s * 18 + 2, _bits(1.2345678))
    key, _ = capi.jit_value_key(sc)
    user, uservals = tmp_path / "user", tmp_path / "user-values"
    out, outvals = tmp_path / "out", tmp_path / "out-values"
    user.mkdir()
    uservals.mkdir()
    cap = 32
    old = []
    for i in range(cap):
        p = uservals / ("%016x.co" % (0x1000 + i))
        p.write_bytes(b"not a code object")
        os.utime(p, (1_000_000 + 10 * i, 1_000_000 + 10 * i))  # oldest first
        old.append(p.name)
    types = []
    for i in range(3):
        p = user / ("%016x.co" % (0x2000 + i))
        p.write_bytes(b"not a code object")
        os.utime(p, (1_000, 1_000))  # older than every value object
        types.append(p.name)
    capi.set_jit_cache(str(user))
    try:
        assert capi.jit_prebuild(sc, cache_dir=str(out))
    finally:
        capi.set_jit_cache(None)
    values = sorted(os.listdir(outvals))
    assert "%s.co" % key in values, (key, values)
    # 16 samples in flight and 1: a types kernel in the directory, a value kernel beside it, each
    assert len(values) == 2 and len(os.listdir(out)) == 2, (values, os.listdir(out))
    blob = (outvals / ("%s.co" % key)).read_bytes()
    assert blob[:8] == b"SAILJIT1" and blob[32:36] == b"\x7fELF" and b"sail_trace_kernel_jit_grouped" in blob
    assert set(types) <= set(os.listdir(user)), "a types kernel's object was deleted"
    have = set(os.listdir(uservals))
    assert len(have) == cap, len(have)
    assert set(values) <= have
    assert [f for f in old if f not in have] == old[:2], "the two oldest value objects go, nothing else"
