"""GPU: the baseline-JPEG decoder (sais_amd/csrc/jpeg.hip) at the edges tests/test_jpeg_gpu.py never reaches: tiny geometries,
hand-built streams (tests/jpeg_build.py), the synchronisation status against the model of the entropy phase
(tests/jpeg_sync_ref.py) and corrupt restart intervals.  Everything is bit-exact against Pillow, or a status value."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_build as jb  # noqa: E402
import jpeg_sync_ref as sync  # noqa: E402
from test_jpeg_edges_host import MODEL_JSON, NAMES, modelled  # noqa: E402
from test_jpeg_host import encode, frame, pillow  # noqa: E402

gpu = pytest.mark.gpu
E_SHORT, E_SYNC, E_RANGE = 8, 16, 32


@pytest.fixture(scope="module")
def dec():
    from sais_amd.jpeg import JpegDecoder
    return JpegDecoder("cuda:0")


def decode(dec, blobs, label=""):
    """-> (statuses of the batch, how many files each path took): every output equals Pillow's."""
    before = dict(dec.stats)
    out = dec.decode(blobs).cpu().numpy()
    for i, b in enumerate(blobs):
        assert np.array_equal(out[i], pillow(b)), (label, i, list(dec.last_status))
    return list(dec.last_status), {k: dec.stats[k] - before[k] for k in before}


# ---- a. tiny geometries: dw <= 2 and dh == 1 in chroma(), np < 4 and misaligned rows in jpeg_color, one MCU, one subsequence ----
TINY = [(1, 1), (2, 2), (8, 8), (1, 5), (3, 4), (5, 3), (16, 2), (2, 16), (9, 17), (17, 33)]


@gpu
@pytest.mark.parametrize("hw", TINY)
@pytest.mark.parametrize("ss", [0, 1, 2])
def test_tiny_geometry_matches_pillow(dec, hw, ss):
    blobs = [encode(frame(*hw, 12, seed=s), quality=q, subsampling=ss) for s, q in enumerate((75, 95))]
    status, took = decode(dec, blobs)
    assert status == [0, 0] and took["gpu"] == 2, (status, took)


@gpu
@pytest.mark.parametrize("ss", [1, 2])
def test_narrow_chroma_planes_are_replicated_not_interpolated(dec, ss):
    """W <= 4 with 4:2:x: the chroma plane is at most 2 samples wide and libjpeg replicates it.  Columns of saturated colour make
    the triangle filter's result differ from replication in every row."""
    for h, w in ((2, 3), (7, 4), (16, 4), (33, 3)):
        a = np.zeros((h, w, 3), np.uint8)
        a[:, : w // 2] = (255, 0, 0)
        a[:, w // 2:] = (0, 0, 255)
        a[::3] = a[::3, ::-1]
        status, took = decode(dec, [encode(a, quality=100, subsampling=ss)])
        assert status == [0], status


# ---- b. hand-built streams --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", NAMES)
def test_hand_built_stream_decodes_on_the_gpu(dec, name):
    b, _ = jb.cached_cases()[name]
    status, took = decode(dec, [b.data], name)
    assert status == [0] and took == {"gpu": 1, "unsupported": 0, "failed": 0}, (status, took)


@gpu
def test_hand_built_streams_in_one_batch(dec):
    """Every 40 x 48 case at once: per-image tables, selectors, sampling and restart intervals inside one launch."""
    blobs = [b.data for b, kw in jb.cached_cases().values() if (kw["H"], kw["W"]) == (40, 48)]
    assert len(blobs) >= 14
    status, took = decode(dec, blobs)
    assert status == [0] * len(blobs) and took["gpu"] == len(blobs), status


@gpu
def test_idct_output_beyond_the_range_limit_table_goes_to_the_host(dec):
    """Coefficients no encoder writes: row-pass output outside [-512, 511], where jidctint.c wraps and the SIMD IDCT saturates."""
    ok = jb.cached_cases()["sel_all0"][0].data
    status, took = decode(dec, [ok, jb.out_of_range_file(), ok])
    assert status == [0, E_RANGE, 0] and took["gpu"] == 2 and took["failed"] == 1, (status, took)


# ---- c. synchronisation bands: the status against the model -----------------------------------------------------------------
def record(name, status):
    rows = json.load(open(MODEL_JSON)) if os.path.exists(MODEL_JSON) else {}
    if rows.get(name, {}).get("gpu_status") != int(status):
        rows.setdefault(name, {})["gpu_status"] = int(status)
        with open(MODEL_JSON, "w") as f:
            json.dump(rows, f, indent=1, sort_keys=True)
            f.write("\n")


def check_band(name, data, status):
    P = modelled(name, data)["passes"]
    want = sync.expected_status(P)
    print(f"{name}: P = {P}, status = {status}, expected {want}")
    record(name, status)
    if want == 0:
        assert status == 0, (name, P, status)
    elif want == E_SYNC:
        assert status & E_SYNC, (name, P, status)
    return want


@gpu
@pytest.mark.parametrize("name", ["noise20_q90_444", "noise40_q95_420"])
def test_files_that_must_synchronise_decode_on_the_gpu(dec, name):
    data, band = jb.sync_cases()[name]
    status, took = decode(dec, [data])
    assert check_band(name, data, status[0]) == 0 and took["gpu"] == 1


@gpu
@pytest.mark.parametrize("name", ["black_420", "shared_tables_444"])
def test_files_that_cannot_synchronise_report_e_sync_and_fall_back(dec, name):
    """A flat 4:2:0 frame (a periodic stream: 32 bits per MCU) and noise whose components share one table pair: a wrong guess never
    corrects itself, the right state crawls from the scan start and MAX_PASSES is far too few.  The file takes the host path."""
    data, band = jb.sync_cases()[name]
    status, took = decode(dec, [data])
    assert check_band(name, data, status[0]) == E_SYNC
    assert took == {"gpu": 0, "unsupported": 0, "failed": 1}, took


@gpu
def test_either_band_file_next_to_a_must_decode_file(dec):
    """128 x 128 uniform noise at q100 (P = 40 by the model) may or may not settle in 32 asynchronous passes: only its pixels are
    checked, and that its status is 0 or E_SYNC alone.  The must-decode file of the same geometry beside it pins a status."""
    data, band = jb.sync_cases()["uniform_q100_444"]
    ok = encode(frame(128, 128, 12), quality=75, subsampling=0)
    status, took = decode(dec, [data, ok])
    assert check_band("uniform_q100_444", data, status[0]) is None and status[0] in (0, E_SYNC)
    assert status[1] == 0 and took["gpu"] + took["failed"] == 2


@gpu
def test_batch_with_must_fail_files_first_middle_and_last_then_a_clean_batch(dec):
    files, bands = jb.batch_files()
    status, took = decode(dec, files)
    for i, (d, band, s) in enumerate(zip(files, bands, status)):
        want = check_band("batch_%d" % i, d, s)
        assert want == (0 if band == "decode" else E_SYNC)
        assert s == want, (i, status)                                         # exactly as predicted: no other bit either
    assert took == {"gpu": 4, "unsupported": 0, "failed": 3}, took
    # the same decoder object, workspace and flags: fewer and shorter files where the failed ones were
    clean = [files[1], files[5], files[2], files[4]]
    status, took = decode(dec, clean)
    assert status == [0] * 4 and took["gpu"] == 4, (status, took)
    status, took = decode(dec, [encode(frame(*jb.BATCH_HW, 12, seed=9), quality=75, restart_marker_blocks=3)])
    assert status == [0], status


# ---- d. corrupt restart intervals ---------------------------------------------------------------------------------------------
@gpu
def test_corrupt_intervals_equal_pillow_or_raise_with_it(dec):
    cases = jb.corrupt_cases()
    valid = {(64, 64): encode(frame(64, 64, 20, seed=1), quality=90, subsampling=0, restart_marker_blocks=2),
             (40, 48): jb.cached_cases()["ri_not_dividing"][0].data, (48, 40): jb.cached_cases()["interval_129"][0].data}
    for name, d in cases.items():
        try:
            want = pillow(d)
        except OSError:
            want = None
        ok = valid[jb.geometry_of(d)]
        if want is None:                                                      # Pillow refuses the file: so does decode()
            with pytest.raises(OSError):
                dec.decode([ok, d])
            continue
        status, took = decode(dec, [ok, d, ok], name)
        assert status[0] == 0 and status[2] == 0, (name, status)              # a file the GPU kept (status 0) equals Pillow too
        assert took == {"gpu": 2 + (status[1] == 0), "unsupported": 0, "failed": int(status[1] != 0)}, (name, took)
        if name.startswith("empty"):
            assert status[1] == E_SHORT, (name, status)
    status, took = decode(dec, [valid[(40, 48)]] * 2)                              # and a valid batch after them
    assert status == [0, 0]
