"""preprocess_kernel (sais_amd/csrc/preprocess.hip) on a real MI355X at every arm of its dispatch: the eight tap-group forms
of the horizontal pass and the byte-wise one, band heights 8, 4, 2 and 1 on both sides of every switch-over, the byte-wise
tail of the dword loader, tiny frames, input that does not start on a dword, a caller's `out` and stream.

Every case is bit for bit against the Pillow pipeline of tests/preprocess_ref.py.  The output lands in a NaN-filled buffer
with a spare frame on each side that must stay NaN; each case is launched twice.  Boxes of more than 100 rows per column run
preprocess_vfirst_kernel (Pillow's pass order there), so every band height runs at W = 8 and at the narrowest width that still
reaches preprocess_kernel.  The cases come from preprocess_ref.py,
where test_preprocess_edges_host.py::test_every_arm_and_band_is_reached proves which arm and band each one reaches."""
import ctypes

import numpy as np
import pytest
import torch

import preprocess_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int32)


def run_guarded(pre, frames_dev, n):
    """the [n, 3, 224, 224] result out of a NaN buffer of n + 2 frames, launched twice; the guards must stay NaN"""
    results = []
    for _ in range(2):
        buf = torch.full((n + 2, 3, 224, 224), float("nan"), dtype=torch.float32, device=DEV)
        got = pre(frames_dev, out=buf[1:n + 1])
        assert got.data_ptr() == buf[1].data_ptr()
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[n + 1]).all()), "wrote outside the output"
        assert not bool(torch.isnan(buf[1:n + 1]).any()), "left part of the output unwritten"
        results.append(buf[1:n + 1].clone())
    assert torch.equal(_bits(results[0]), _bits(results[1])), "two launches differ"
    return results[0].cpu().numpy()


def check_case(c, kind, seed=0):
    from sais_amd.preprocess import FramePreprocessor
    frames = R.make_frames(kind, c.F, c.H, c.W, seed)
    want = np.stack([R.pil_pipeline(f, c.hf, c.wf) for f in frames])
    pre = FramePreprocessor(c.H, c.W, c.hf, c.wf)
    try:
        i = c.info
        assert pre.box == (i["left"], i["top"], i["left"] + i["cw"], i["top"] + i["ch"])
        dev = torch.from_numpy(frames).to(DEV)                     # its own allocation: the last frame ends it
        assert dev.data_ptr() % 4 == 0
        got = run_guarded(pre, dev, c.F)
    finally:
        pre.close()
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, f"{c} {kind}: {len(bad)} values differ from Pillow, first at [f, c, y, x] = {bad[0].tolist()}"


@pytest.mark.parametrize("case,kind", R.case_kinds(), ids=lambda v: str(v))
def test_bit_exact_against_pillow(case, kind):
    check_case(case, kind, seed=case.H * 7 + case.W)


def test_flat_255_stays_255_on_every_arm():
    """The coefficient rows of both axes sum so that a white frame stays white: the value Normalize gives byte 255."""
    from oracle import preprocess_oracle as po
    white = po.normalize_lut()[:, 255]
    from sais_amd.preprocess import FramePreprocessor
    for c in [c for c, k in R.case_kinds() if k == "flat" and c in R.TAP_CASES]:
        pre = FramePreprocessor(c.H, c.W, c.hf, c.wf)
        try:
            got = pre(torch.full((1, c.H, c.W, 3), 255, dtype=torch.uint8, device=DEV)).cpu().numpy()
        finally:
            pre.close()
        for ch in range(3):
            assert (got[0, ch] == white[ch]).all(), c


def test_first_refused_height_raises_and_leaves_no_plan():
    from sais_amd import _lib as L
    from sais_amd.preprocess import FramePreprocessor
    c = R.refused_case()
    plan = ctypes.c_void_p()
    m, s = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.25, 0.25, 0.25)
    rc = L.load().sais_preprocess_plan_create(c.H, c.W, c.hf, c.wf, ctypes.cast(m, ctypes.c_void_p),
                                              ctypes.cast(s, ctypes.c_void_p), ctypes.byref(plan))
    assert rc == -1 and not plan.value
    with pytest.raises(L.SaisHipError):
        FramePreprocessor(c.H, c.W, c.hf, c.wf)


@pytest.mark.parametrize("H,W,F", [(5, 3, 3), (7, 5, 2), (3, 227, 2)])
def test_input_that_does_not_start_on_a_dword(H, W, F):
    """The same frames at byte offsets 1, 2 and 3 of a uint8 buffer: FramePreprocessor copies them and gives the bytes of the
    aligned run; the raw entry refuses the pointer."""
    from sais_amd import _lib as L
    from sais_amd.preprocess import FramePreprocessor
    frames = R.make_frames("random", F, H, W, seed=H + W)
    want = np.stack([R.pil_pipeline(f, 1.0, 1.0) for f in frames])
    n = frames.size
    pre = FramePreprocessor(H, W, 1.0, 1.0)
    try:
        aligned = run_guarded(pre, torch.from_numpy(frames).to(DEV), F)
        assert np.array_equal(aligned.view(np.int32), want.view(np.int32))
        for off in (1, 2, 3):
            buf = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device=DEV)
            assert buf.data_ptr() % 4 == 0
            view = buf[off:off + n].view(F, H, W, 3)
            view.copy_(torch.from_numpy(frames))
            assert view.data_ptr() % 4 == off and view.is_contiguous()
            got = run_guarded(pre, view, F)
            assert np.array_equal(got.view(np.int32), aligned.view(np.int32)), off
            out = torch.full((F, 3, 224, 224), float("nan"), dtype=torch.float32, device=DEV)
            rc = L.load().sais_preprocess_run(pre._plan, view.data_ptr(), F, out.data_ptr(), None)
            torch.cuda.synchronize()
            assert rc == -1 and bool(torch.isnan(out).all()), off
        # a slice of a batch whose frames are not a multiple of 4 bytes long starts inside a dword
        if (H * W * 3) % 4:
            batch = torch.from_numpy(frames).to(DEV)
            assert batch[1:].data_ptr() % 4 != 0
            got = run_guarded(pre, batch[1:], F - 1)
            assert np.array_equal(got.view(np.int32), want[1:].view(np.int32))
    finally:
        pre.close()


def test_caller_out_and_stream():
    from sais_amd.preprocess import FramePreprocessor
    c = R.Case("stream", 37, 301, F=3, hf=0.8, wf=0.7)
    frames = R.make_frames("random", c.F, c.H, c.W, seed=5)
    want = np.stack([R.pil_pipeline(f, c.hf, c.wf) for f in frames])
    pre = FramePreprocessor(c.H, c.W, c.hf, c.wf)
    try:
        dev = torch.from_numpy(frames).to(DEV)
        out = torch.full((c.F, 3, 224, 224), float("nan"), dtype=torch.float32, device=DEV)
        assert pre(dev, out=out) is out
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = run_guarded(pre, dev, c.F)
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
        with pytest.raises(ValueError):
            pre(dev, out=out[:2])
        with pytest.raises(ValueError):
            pre(dev, out=out.double())
    finally:
        pre.close()
