"""CPU-only: every hand-built file of tests/jpeg_build.py is legal (Pillow and tests/jpeg_ref.py decode it to the same pixels,
sais_jpeg_parse accepts it with the selectors and tables the case intended) and reaches the edge it was built for; the model of the
entropy phase (tests/jpeg_sync_ref.py) converges to the sequential decode's states and puts the synchronisation cases of
tests/test_jpeg_edges_gpu.py in their bands.  The model's table goes to profiles/jpeg_sync_model.json."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_build as jb  # noqa: E402
import jpeg_ref  # noqa: E402
import jpeg_sync_ref as sync  # noqa: E402
from test_jpeg_host import lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_JSON = os.path.join(ROOT, "profiles", "jpeg_sync_model.json")

NAMES = ("lengths_1_9_10_16", "one_bit_blocks", "sel_y1_c0", "sel_cross", "sel_all0", "quant_3_tables", "sof1", "pq1", "extremes",
         "runs_and_zrl", "dense_ff", "ri_1", "ri_not_dividing", "ri_row_plus_1", "ri_ge_mcus", "ri_above_mcus", "interval_127",
         "interval_128", "interval_129", "interval_256", "interval_1_byte")


def coefficient_stats(data):
    """(largest DC difference category, largest AC category, longest zero run, AC count of the fullest block) of a file."""
    hd = jpeg_ref.parse(data)
    co = jpeg_ref.coefficients(data, hd)
    zz = [c.reshape(-1, 64)[:, jpeg_ref.ZIGZAG] for c in co]
    ac = np.concatenate([z[:, 1:] for z in zz])
    runs = 0
    for row in ac:
        nzi = np.flatnonzero(row)
        if len(nzi):
            runs = max(runs, int(np.diff(np.concatenate([[-1], nzi])).max()) - 1)
    return int(np.abs(ac).max()), runs, int((ac != 0).sum(1).max())


def first_sub_blocks(data):
    L = sync.Layout(data)
    return L.run(L.sego[0] * 8, 0, 0, L.sego[0] * 8 + sync.SUB_BITS)[3]


EDGES = {
    "lengths_1_9_10_16": lambda b: {(c, n) for c in (0, 1) for n in (1, 9, 10, 16)} <= b.used and max(n for _, n in b.used) == 16,
    "one_bit_blocks": lambda b: first_sub_blocks(b.data) >= 400,
    "sel_y1_c0": lambda b: True, "sel_cross": lambda b: True, "sel_all0": lambda b: b.data.count(b"\xff\xc4") == 1,
    "quant_3_tables": lambda b: b.data.count(b"\xff\xdb") == 3,
    "sof1": lambda b: b"\xff\xc1" in b.data and b"\xff\xc0" not in b.data,
    "pq1": lambda b: b.data[b.data.find(b"\xff\xdb") + 4] >> 4 == 1,
    "extremes": lambda b: coefficient_stats(b.data)[0] == 1023 and coefficient_stats(b.data)[2] == 63 and (0, 9) in b.used,
    "runs_and_zrl": lambda b: coefficient_stats(b.data)[1] == 62,
    "dense_ff": lambda b: all(jb.ff_edges(b)[k] >= 1 for k in ("last", "boundary", "pairs")) and jb.ff_edges(b)["stuffed"] >= 100
    and b"\xff\xff\xff\xff\xd0" in b.data and b.data.endswith(b"\xff\xff\xff\xd9"),
    "ri_1": lambda b: len(b.lens) == 30 and b"\xff\xd7\xff" not in b.data[:20] and b.data.count(b"\xff\xd0") >= 3,
    "ri_not_dividing": lambda b: len(b.lens) == 8 and 30 % 4,
    "ri_row_plus_1": lambda b: len(b.lens) == 5,
    "ri_ge_mcus": lambda b: len(b.lens) == 1 and b"\xff\xdd\x00\x04\x00\x09" in b.data,
    "ri_above_mcus": lambda b: len(b.lens) == 1 and b"\xff\xdd\x00\x04\x01\xf4" in b.data,
    "interval_127": lambda b: b.lens[1] == 127, "interval_128": lambda b: b.lens[1] == 128,
    "interval_129": lambda b: b.lens[1] == 129, "interval_256": lambda b: b.lens[1] == 256,
    "interval_1_byte": lambda b: b.lens[1:] == [1] * 29,
}


def test_the_matrix_is_the_one_the_tests_name():
    assert set(jb.cached_cases()) == set(NAMES) == set(EDGES)


@pytest.mark.parametrize("name", NAMES)
def test_built_file_is_legal_and_reaches_its_edge(name):
    lib()
    from sais_amd import jpeg
    b, kw = jb.cached_cases()[name]
    want = jb.pillow(b.data)
    assert want.shape == (kw["H"], kw["W"], 3)
    assert np.array_equal(jpeg_ref.decode(b.data), want)
    rc, hd = jpeg.parse_rc(b.data)
    assert rc == 0
    assert (hd.height, hd.width) == (kw["H"], kw["W"]) and (hd.hsamp, hd.vsamp) == jb.SAMPLING[kw["sub"]]
    assert tuple(hd.dcsel) == tuple(kw.get("dcsel", (0, 1, 1))) and tuple(hd.acsel) == tuple(kw.get("acsel", (0, 1, 1)))
    assert tuple(hd.qsel) == tuple(kw.get("qsel", (0, 1, 1)))
    assert hd.restart_interval == kw.get("ri", 0) and hd.segments == len(b.lens)
    quant = kw.get("quant", {0: np.full(64, 3), 1: np.full(64, 5)})
    for t, q in quant.items():
        assert list(hd.quant[t]) == list(q)
    assert hd.scan_offset + hd.scan_bytes == len(b.data)
    L = sync.Layout(b.data)                                                   # the model's destuffing agrees with the builder
    assert [e - o for o, e in zip(L.sego, L.sege)] == b.lens
    assert EDGES[name](b), name


def test_zrl_past_the_block_end_closes_the_block_without_an_eob():
    """Block 3 of runs_and_zrl ends in a ZRL at k = 51: the bytes differ from the standard encoding (which would write an EOB) and
    the decoded coefficients do not."""
    b, kw = jb.cached_cases()["runs_and_zrl"]
    kw = {k: v for k, v in kw.items() if k not in ("H", "W", "sub", "raw_ac")}
    blocks = jb.noise_blocks(40, 48, 2, 3, 9, nz=0.1)
    blocks[0:4, 1:] = 0
    blocks[0, 16], blocks[1, 17], blocks[2, 63], blocks[3, 50] = 2, -3, 1, 4
    std = jb.build(40, 48, blocks, 2, **kw)
    assert std.data != b.data
    for x, y in zip(jpeg_ref.coefficients(std.data), jpeg_ref.coefficients(b.data)):
        assert np.array_equal(x, y)


def test_spec_helper_accepts_what_libjpeg_accepts():
    for counts, symbols in jb.STD_HUFF.values():
        jb.check_spec(counts)
    assert jb.spec_from_lengths((5, 6, 7), [3, 1, 2]) == ((1, 1, 1) + (0,) * 13, (6, 7, 5))
    for bad in ([2] + [0] * 15,                   # both 1-bit codes: the all-ones code in use
                [1, 2] + [0] * 14,                # Kraft sum 1: 0, 10, 11
                [0, 0, 8] + [0] * 13,             # code + count = 2^l at l = 3
                [0] * 15 + [256]):                # a count beyond a byte
        with pytest.raises(AssertionError):
            jb.check_spec(bad)
        # libjpeg says the same of the first three (the fourth cannot be written)
    dc, ac = jb._lengths_tables()
    assert sum(dc[0]) == 12 and sum(ac[0]) == 162


def test_out_of_range_and_corrupt_files_pass_the_parser():
    lib()
    from sais_amd import jpeg
    assert jpeg.parse_rc(jb.out_of_range_file())[0] == 0
    for name, d in jb.corrupt_cases().items():
        assert jpeg.parse_rc(d)[0] == 0, name


_MODEL = {}


def modelled(name, data):
    if name not in _MODEL:
        _MODEL[name] = sync.model(data)
    return _MODEL[name]


def sync_matrix():
    files = {name: (d, band) for name, (d, band) in jb.sync_cases().items()}
    batch, bands = jb.batch_files()
    for i, (d, band) in enumerate(zip(batch, bands)):
        files["batch_%d" % i] = (d, band)
    return files


def test_model_converges_to_the_sequential_decode():
    files = {n: d for n, (d, _) in sync_matrix().items()}
    for name in ("ri_not_dividing", "ri_row_plus_1", "interval_128", "interval_256", "dense_ff", "one_bit_blocks"):
        files[name] = jb.cached_cases()[name][0].data
    for name, d in files.items():
        m = modelled(name, d)
        seq = sync.sequential(m["layout"])
        assert m["entries"] == seq, name
        assert m["subsequences"] == sum(-(-(e - o) // sync.SUB_BYTES) for o, e in zip(m["layout"].sego, m["layout"].sege))


def test_sync_cases_fall_in_their_bands_and_table_is_written():
    rows, per_band = {}, {"decode": 0, "fail": 0, "either": 0}
    for name, (d, band) in sync_matrix().items():
        m = modelled(name, d)
        P = m["passes"]
        rows[name] = dict(band=band, bytes=len(d), subsequences=m["subsequences"], wrong_guesses=m["wrong_guesses"], passes=P)
        if band == "decode":
            assert P <= 20 and sync.expected_status(P) == 0, (name, P)
        elif band == "fail":
            assert P >= sync.MUST_FAIL_P and sync.expected_status(P) == sync.E_SYNC, (name, P)
        else:
            assert sync.expected_status(P) is None, (name, P)
        if not name.startswith("batch_"):
            per_band[band] += 1
    assert per_band["decode"] >= 2 and per_band["fail"] >= 2 and per_band["either"] <= 2
    assert max(r["wrong_guesses"] for r in rows.values() if r["band"] == "decode") > 0    # a decode case that needs passes
    old = {}
    if os.path.exists(MODEL_JSON):
        old = json.load(open(MODEL_JSON))
    for name, row in rows.items():                                            # the GPU test's columns stay
        row.update({k: v for k, v in old.get(name, {}).items() if k.startswith("gpu_")})
    if rows != old:
        with open(MODEL_JSON, "w") as f:
            json.dump(rows, f, indent=1, sort_keys=True)
            f.write("\n")
