"""No-GPU check of csrc/philox.h, the one header the draws of the playback chain come from ("The playback chain"):
tests/hip/philox_host.cpp, a stand-alone program over the header built with the host C++ compiler, against the references the GPU
draw tests compare the device with (place_ref / rir_ref / chan_ref) on those tests' arguments, and the disjointness of the four
Philox streams as the header's own table lays them out.  The same queries run once more through an UBSan + ASan build."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import chan_ref as CR
import place_ref as PR
import rir_ref as RR

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hip", "philox_host.cpp")
SEED, BASE = 5, 7
OTHER = SEED + (1 << 32)          # the seed the GPU tests pair with the evaluation stream


def _compiler():
    for c in (shutil.which("c++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and os.path.exists(c):
            return c
    pytest.fail("no host C++ compiler: neither c++ nor ROCm's clang++")


def _build(tmp, name, *flags):
    exe = str(tmp / name)
    r = subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", *flags, "-o", exe, SRC], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("philox"), "philox_host")


def ask(exe, queries):
    """One line of tokens per query."""
    r = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert len(lines) == len(queries)
    return lines


KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def _philox_queries():
    return ["philox " + " ".join(str(x) for x in c + k) for c, k, _ in KNOWN]


def test_philox_known_answers(exe):
    for (c, k, want), got in zip(KNOWN, ask(exe, _philox_queries())):
        assert " ".join(got) == want
        assert " ".join(f"{w:08x}" for w in PR.philox4x32_10(c, k)) == want


PLACE = [(seed, step, stream, Lp, on, G) for seed, stream in ((SEED, 0), (OTHER, 1)) for Lp in (1, 1000, 16000)
         for on, G in ((1, 0.0), (1, 6.0), (0, 6.0)) for step in range(3)]
ROOM = [(seed, step, stream, N) for seed, stream in ((SEED, 0), (OTHER, 1)) for N in (1, 3, 64) for step in range(3)]
CHAN = [(seed, step, stream, B, D) for seed, stream in ((SEED, 0), (OTHER, 1)) for B in (5, 300) for D in (CR.drift_q32(20000.0), 0)
        for step in (0, 3, 4)]
LO, HI = 12.5, 30.0


def _draw_queries():
    return [f"place {s} {st} {BASE} 5 {sm} {Lp} {on} {G}" for s, st, sm, Lp, on, G in PLACE] \
        + [f"room {s} {st} {BASE} 5 {sm} {N}" for s, st, sm, N in ROOM] \
        + [f"chan {s} {st} {BASE} {B} {sm} {D} {LO} {HI}" for s, st, sm, B, D in CHAN]


def test_draws_equal_the_references(exe):
    got = ask(exe, _draw_queries())
    for (s, st, sm, Lp, on, G), row in zip(PLACE, got):
        s_ref, a_ref = PR.draw(s, st, BASE, 5, sm, Lp, bool(on), G)
        assert [int(x) for x in row[0::2]] == s_ref.tolist(), (s, st, sm, Lp, on, G)
        a = np.array([float(x) for x in row[1::2]])
        assert np.all(a == 1.0) if G == 0.0 else np.all(np.abs(a - a_ref) <= 1e-6 * a_ref)
    for (s, st, sm, N), row in zip(ROOM, got[len(PLACE):]):
        assert [int(x) for x in row] == RR.draw(s, st, BASE, 5, sm, N).tolist(), (s, st, sm, N)
    for (s, st, sm, B, D), row in zip(CHAN, got[len(PLACE) + len(ROOM):]):
        want_rq, want_snr = CR.draw(s, st, BASE, B, sm, D, LO, HI)
        assert [int(x) for x in row[0::2]] == want_rq, (s, st, sm, B, D)
        snr = np.array([float(x) for x in row[1::2]])
        assert np.all(np.abs(snr - want_snr.astype(np.float64)) <= np.spacing(np.abs(want_snr).astype(np.float32)))
        assert D or want_rq == [1 << 32] * B


GRID = [(seed, step, clip, stream) for seed in (0, 5, (1 << 64) - 1, CR.NOISE_KEY << 32) for step in range(3) for clip in range(3)
        for stream in range(3)]


def _table_queries():
    return [f"input {name} {seed} {step} {clip} {stream} {g}" for seed, step, clip, stream in GRID
            for name, groups in (("place", 1), ("room", 1), ("chan", 1), ("noise", 4)) for g in range(groups)]


def test_streams_of_the_table_are_disjoint(exe):
    """No (counter, key) pair is shared between the four streams, and the header's layout is the references'."""
    rows = iter(ask(exe, _table_queries()))
    owner = {}
    for seed, step, clip, stream in GRID:
        for name, groups in (("place", 1), ("room", 1), ("chan", 1), ("noise", 4)):
            for g in range(groups):
                w = tuple(int(x) for x in next(rows))
                pair = (w[:4], w[4:])
                tag = {"place": CR.TAG_PLACE, "room": CR.TAG_ROOM, "chan": CR.TAG_CHAN}.get(name)
                want = (CR.noise_counter(step, clip, g, stream), CR.key_of(seed, True)) if tag is None else \
                    ((step, clip, stream, tag), CR.key_of(seed))
                assert pair == want, (name, seed, step, clip, stream, g)
                assert owner.setdefault((seed, pair), name) == name, (name, owner[(seed, pair)], pair)
    names = list(owner.values())
    assert names.count("place") == names.count("room") == names.count("chan") == 4 * 27 and names.count("noise") == 4 * 108


def _normal_queries():
    return [f"normal {SEED} 2 {BASE} 1 61"]


def test_normal_pair_against_float64(exe):
    """The host build's Box-Muller (libm's cosf / sinf of 2 pi u2) against chan_ref.noise64: the rounding of the angle to float32
    (half a unit of [4, 8): 2^-22), one unit each for cosf / sinf, rad and the product, all scaled by rad — 2^-20 rad bounds them
    twice over."""
    z = np.array([float(x) for x in ask(exe, _normal_queries())[0]])
    u1, _ = CR.noise_uniforms(SEED, 2, BASE, 1, 61)
    want = CR.noise64(SEED, 2, BASE, 1, 61)
    assert z.shape == want.shape and np.all(np.abs(z - want) <= 2.0 ** -20 * np.sqrt(-2.0 * np.log(u1)))


def test_every_query_under_the_sanitizers(exe, tmp_path):
    """The same program with -fsanitize=undefined,address (stand-alone, so nothing is preloaded): no report, the same answers."""
    san = _build(tmp_path, "philox_host_san", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all")
    q = _philox_queries() + _draw_queries() + _table_queries() + _normal_queries()
    assert ask(san, q) == ask(exe, q)
