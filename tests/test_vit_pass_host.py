"""CPU-only: which form VisionTransformer._pass_form gives a backbone pass (resident, streaming, segmented: sais_amd/vit.py), from
what _forward_kernels receives, and the texts it refuses an impossible combination with.  Shapes only: nothing is launched."""
import pytest
import torch

from sais_amd.vit import VisionTransformer, _GroupPass, _SegPass, vit_small
from sais_amd.vit_seg import SegPlan

SEG_TEXT = "the segmented pass is the patch-16 streaming pass to the last block or the final norm"


@pytest.fixture(scope="module")
def m16():
    return vit_small(depth=1)


@pytest.fixture(scope="module")
def m8():
    return vit_small(patch_size=8, depth=1)


def frames(*shapes):
    return [torch.empty(n, 3, H, W) for n, H, W in shapes]


def plan(imgs):
    """VisionTransformer._seg_plan without the copy to a device: one segment per frame, in list order."""
    return SegPlan([(im.shape[2] // 16, im.shape[3] // 16) for im in imgs for _ in range(im.shape[0])])


def form_of(model, imgs, streaming=None, seg=None, end="reps"):
    """The form as the public methods ask for it: forward() and the multi-crop pass decide `streaming` with streaming_pass."""
    streaming = VisionTransformer.streaming_pass(imgs) if streaming is None else streaming
    form, as_list = model._pass_form(imgs if len(imgs) > 1 else imgs[0], streaming, seg, end)
    assert [tuple(a.shape) for a in as_list] == [tuple(a.shape) for a in imgs]
    return form


@pytest.mark.parametrize("shapes", [((2, 224, 224),), ((3, 96, 96),), ((2, 224, 224), (5, 96, 96)), ((1, 96, 96), (1, 224, 224))])
def test_square_sides_give_a_resident_pass(m16, shapes):
    imgs = frames(*shapes)
    form = form_of(m16, imgs)
    assert type(form) is _GroupPass and not form.streaming and form.resident and form.seg is None
    assert form.one_call == (len(shapes) == 1)
    assert [(g["Fr"], g["ntok"]) for g in form.groups] == [(n, 1 + (H // 16) * (W // 16)) for n, H, W in shapes]
    assert form.M == sum(n * (1 + (H // 16) * (W // 16)) for n, H, W in shapes)
    assert form.NP == form.M - form.Ftot and form.Ftot == sum(n for n, _, _ in shapes)
    assert form.cls_only(save=True) and form.cls_only(save=False)


@pytest.mark.parametrize("shapes", [((2, 64, 96),), ((1, 224, 240),), ((1, 96, 224),), ((2, 128, 128),), ((1, 16, 16),),
                                    ((2, 224, 224), (3, 96, 128)), ((1, 480, 832),)])
def test_any_other_shape_gives_a_streaming_pass(m16, shapes):
    form = form_of(m16, frames(*shapes))
    assert type(form) is _GroupPass and form.streaming and not form.resident and not form.one_call and form.seg is None
    # a saved pass keeps the CLS-only last block only while the one-wave CLS backward holds every group (200 tokens)
    assert form.cls_only(save=False)
    assert form.cls_only(save=True) == all(1 + (H // 16) * (W // 16) <= 200 for _, H, W in shapes)


def test_the_inference_entries_stream_at_224_too(m16):
    form = form_of(m16, frames((2, 224, 224)), streaming=True, end="blocks")      # dense_features, retrieval_features, cls_attention
    assert type(form) is _GroupPass and form.streaming and not form.one_call


@pytest.mark.parametrize("shape", [(2, 224, 224), (1, 96, 96), (2, 64, 96), (1, 8, 8), (1, 448, 112)])
@pytest.mark.parametrize("end", ["reps", "blocks", "norm1"])
def test_every_patch8_pass_is_streaming(m8, shape, end):
    """Every public method of a patch-8 model passes streaming=True (forward, probe_features, get_intermediate_layers,
    dense_features, retrieval_features, cls_attention); the rows are counted in 8 x 8 patches."""
    form = form_of(m8, frames(shape), streaming=True, end=end)
    n, H, W = shape
    assert type(form) is _GroupPass and form.streaming and not form.resident and not form.one_call
    assert form.M == n * (1 + (H // 8) * (W // 8)) and form.Ftot == n


def test_patch8_public_methods_ask_for_streaming(m8, monkeypatch):
    asked = []

    class Stop(Exception):
        pass

    def pass_form(img, streaming, seg, end):
        asked.append((streaming, seg, end))
        raise Stop

    monkeypatch.setattr(m8, "_pass_form", pass_form)
    monkeypatch.setattr(m8, "_engine", lambda device: None)
    monkeypatch.setattr(m8, "_check_input", lambda x, any_size=None: x)
    x = torch.empty(1, 3, 64, 96)
    calls = [lambda: m8(x), lambda: m8.dense_features(x), lambda: m8.get_intermediate_layers(x), lambda: m8.probe_features(x, 1),
             lambda: m8.probe_features(x, 1, avgpool=True), lambda: m8.cls_attention(x), lambda: m8.retrieval_features(x),
             lambda: m8.retrieval_features(x, cls_only=True)]
    with torch.no_grad():
        for call in calls:
            with pytest.raises(Stop):
                call()
    assert len(asked) == len(calls) and all(s is True and seg is None for s, seg, _ in asked)


@pytest.mark.parametrize("end", ["blocks", "reps"])
def test_a_plan_gives_a_segmented_pass(m16, end):
    imgs = frames((1, 224, 224), (2, 64, 96), (1, 160, 272))
    seg = plan(imgs)
    form = form_of(m16, imgs, streaming=True, seg=seg, end=end)
    assert type(form) is _SegPass and form.seg is seg and form.streaming and not form.resident and not form.one_call
    assert (form.M, form.NP, form.Ftot) == (seg.M, seg.NP, seg.nseg) == (197 + 2 * 25 + 171, 196 + 2 * 24 + 170, 4)
    assert not form.cls_only(save=False) and not form.cls_only(save=True)
    rec = form.record()
    assert rec["form"] is form and rec["seg"] is seg and rec["streaming"] is True and (rec["M"], rec["Ftot"]) == (seg.M, 4)
    assert [(g["Fr"], g["ntok"], g["off"]) for g in rec["groups"]] == [(1, 197, 0), (2, 25, 197), (1, 171, 247)]


@pytest.mark.parametrize("streaming,end", [(False, "reps"), (False, "blocks"), (True, "probs"), (True, "norm1"), (False, "probs"),
                                           (False, "norm1")])
def test_every_other_pair_with_a_plan_is_refused(m16, streaming, end):
    imgs = frames((2, 64, 96))
    with pytest.raises(NotImplementedError) as e:
        form_of(m16, imgs, streaming=streaming, seg=plan(imgs), end=end)
    assert str(e.value) == SEG_TEXT


def test_a_plan_is_refused_on_patch8_and_on_other_rows(m16, m8):
    imgs = frames((1, 64, 96), (1, 32, 32))
    with pytest.raises(NotImplementedError) as e:
        form_of(m8, imgs, streaming=True, seg=plan(imgs), end="blocks")
    assert str(e.value) == SEG_TEXT
    for other in (plan(imgs[:1]), plan(frames((1, 64, 96), (1, 32, 48))), plan(frames((2, 64, 96), (1, 32, 32)))):
        assert other.M != plan(imgs).M
        with pytest.raises(NotImplementedError) as e:
            form_of(m16, imgs, streaming=True, seg=other, end="blocks")       # seg.M must equal the stacked row count
        assert str(e.value) == SEG_TEXT


def test_probabilities_take_one_resolution(m16):
    imgs = frames((1, 224, 224), (1, 96, 96))
    for seg in (None, plan(imgs)):                 # (the resolution check comes first, as before the forms)
        with pytest.raises(ValueError) as e:
            form_of(m16, imgs, streaming=seg is not None, seg=seg, end="probs")
        assert str(e.value) == "get_last_selfattention takes one resolution"
    assert type(form_of(m16, imgs[:1], end="probs")) is _GroupPass


def test_a_grouped_record_keeps_the_keys_other_modules_read(m16):
    rec = form_of(m16, frames((2, 224, 224), (3, 96, 96))).record()
    assert set(rec) == {"form", "groups", "M", "Ftot", "streaming", "seg"} and rec["seg"] is None and rec["streaming"] is False
    assert [(g["Fr"], g["ntok"], g["off"]) for g in rec["groups"]] == [(2, 197, 0), (3, 37, 394)]
