#!/usr/bin/env python3
"""Which library calls does the host code issue, with which arguments?  For refactors of the host path (sais_amd/*.py): the
log of a tree is compared entry by entry with the log of its parent.

    tools/host_call_log.py --root <tree> --out log.json                 record, no GPU needed (one fresh process per tree)
    tools/host_call_log.py --root <tree> --real --out results.pt        run the temporal / run_windows cases on the GPU, keep results
    tools/host_call_log.py --compare parent.json new.json [--json f]    logs equal?  (.pt: bit-equal, or max |difference|)

Recording replaces `sais_amd._lib.call` by a function that appends (entry name, arguments) to a list and launches nothing.
An argument is logged as: an integer / float as itself; a struct (by value, `byref`, array of, or pointer + the count that
follows it) field by field; a pointer as the ORDER OF ITS FIRST APPEARANCE in the case (0, 1, 2 ...), so two logs agree when the
same buffers play the same roles, whatever their addresses.  Every tensor whose pointer was logged is kept alive until the case
ends (`ops._p` is wrapped), so an address is never handed out twice and equal numbers mean equal buffers.  `KernelTimer` tags
are logged with their flops / bytes (`ops._timed` is wrapped), gradient hooks log their arguments into the same list.

How device tensors are stood in for without a GPU: the cases run on CPU tensors.  `torch.Tensor.is_cuda` is overridden to
answer True (the package refuses host tensors), `ops._stream()` gives NULL, `torch.cuda.is_current_stream_capturing()` and
`torch.cuda.is_available()` are constants; `vit_seg.SegPlan.to_device` logs the sha256 of the plan's host buffer (so the plan's
contents are part of the record) and stands a CPU tensor over the same bytes in for the device copy.  Nothing is computed, so outputs hold whatever `torch.empty` returned: no host
decision of the package depends on a kernel's result.  The pure host functions of the library (`sais_tgemm_nsplit`,
`sais_workspace_bytes`, ...) are the real ones: the library must be built, it is only never asked to launch.
Only names that bench.py, the tests and tools/ rely on are used, so the same file runs against older trees.
"""
import argparse
import ctypes
import json
import os
import sys


class Recorder:
    def __init__(self):
        self.log, self.ids, self.keep = [], {}, []

    def reset(self):
        self.log, self.ids, self.keep = [], {}, []

    def ptr(self, v):
        if not v:
            return None
        return "p%d" % self.ids.setdefault(int(v), len(self.ids))

    def enc(self, a, count=None):
        if a is None or isinstance(a, (bool, int, str)):
            return a
        if isinstance(a, float):
            return repr(a)
        if isinstance(a, ctypes.c_void_p):
            return self.ptr(a.value)
        if type(a).__name__ == "CArgObject":                         # ctypes.byref(x)
            return self.enc(a._obj)
        if isinstance(a, ctypes.Structure):
            out = {}
            for name, typ in a._fields_:
                v = getattr(a, name)
                out[name] = self.ptr(v) if typ is ctypes.c_void_p else self.enc(v)
            return out
        if isinstance(a, ctypes.Array):
            if a._type_ is ctypes.c_void_p:
                return [self.ptr(v) for v in a]
            return [self.enc(v) for v in a]
        if isinstance(a, ctypes._Pointer):
            return [self.enc(a[i]) for i in range(count)] if count is not None else (self.enc(a.contents) if a else None)
        if isinstance(a, (ctypes.c_int, ctypes.c_long, ctypes.c_uint, ctypes.c_float, ctypes.c_double)):
            return self.enc(a.value)
        raise TypeError(f"host_call_log: argument of type {type(a)}")

    def call(self, name, *args):
        row = [name]
        for i, a in enumerate(args):
            n = args[i + 1] if isinstance(a, ctypes._Pointer) and i + 1 < len(args) and isinstance(args[i + 1], int) else None
            row.append(self.enc(a, n))
        self.log.append(row)
        return 0


REC = Recorder()


def install_recorder():
    import hashlib
    import torch
    from sais_amd import _lib, ops, vit_seg
    _lib.call = REC.call
    real_p, real_items = ops._p, ops.tn_items

    def _p(t):
        if t is not None:
            REC.keep.append(t)
        return real_p(t)

    def tn_items(n):
        arr = real_items(n)
        REC.keep.append(arr)
        return arr

    def _timed(tag, flops, nbytes, fn):
        if ops.TIMER is not None:
            REC.log.append(["timer", tag, repr(float(flops)), int(nbytes)])
        fn()

    def to_device(plan, device):                 # the plan's contents are part of the record; no pinned copy without a GPU
        REC.log.append(["segplan", hashlib.sha256(plan.host.tobytes()).hexdigest()])
        plan.dev = torch.from_numpy(plan.host)
        return plan

    vit_seg.SegPlan.to_device = to_device
    ops._p, ops.tn_items, ops._timed, ops._stream = _p, tn_items, _timed, lambda: None
    torch.Tensor.is_cuda = property(lambda self: True)
    torch.cuda.is_current_stream_capturing = lambda: False
    torch.cuda.is_available = lambda: True


# ------------------------------------------------------------------------------------------------ cases
CASES = []            # (name, function(dev) -> results or None, runs in --real mode)


def case(name, real=False):
    def deco(fn):
        CASES.append((name, fn, real))
        return fn
    return deco


def _engine_events(m, dev, names_of_t, sentinel):
    """The event sequence of the freshness rules: first / second _engine call, in-place edit, load_state_dict, re-pointed
    parameter.  Each event is a marker row in the log, followed by what the next _engine call launched."""
    import torch
    for what in ("first", "second", "edit", "load_state_dict", "rebuilt"):
        if what == "edit":
            with torch.no_grad():
                dict(m.named_parameters())[sentinel].mul_(1.0)
        elif what == "load_state_dict":
            m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
        elif what == "rebuilt":
            p = next(m.parameters())
            p.data = p.data.clone()
        REC.log.append(["event", what])
        m._engine(dev)
    return m


def _temporal(dev, mod="RGB-Flow", ns=1, Tx=6, Tf=6, p=0.1, layer_calls=True, timer=False, dw_defer=True, il=False,
              domain="NH_02", hook=False, xgrad=False, B=2, pads=False):
    import torch
    from sais_amd import ops, temporal as T
    m = T.fullModel('reps', 2, domain, 384, 'ViT', modalities=mod, importance_loss=il).to(dev)
    m.dropout_p = p
    m.train()
    old = T._LAYER_CALLS, T._DW_DEFER, ops.TIMER
    T._LAYER_CALLS, T._DW_DEFER = layer_calls, dw_defer
    if timer:
        ops.TIMER = ops.KernelTimer()
    if hook:
        m.grad_ready_hook = lambda lo, hi: REC.log.append(["hook", lo, hi])
    try:
        g = torch.Generator().manual_seed(3)
        x = torch.randn(B, ns, Tx, 384, generator=g).to(dev).requires_grad_(xgrad) if mod != "Flow" else None
        f = torch.randn(B, ns, Tf, 384, generator=g).to(dev).requires_grad_(xgrad) if mod != "RGB" else None
        xpad = fpad = None
        if pads:
            xpad = torch.zeros(B, ns, Tx + 1, dtype=torch.bool)
            xpad[-1, :, -2:] = True
            fpad = torch.zeros(B, ns, Tf + 1, dtype=torch.bool)
            fpad[0, :, -1:] = True
        domains = ["NH_02", "other"][:B] if "+" in domain else None
        res = []
        for step in range(2):                                        # the second step sees the shadows an sgd_step left
            out = m(x, f, None, None, 'Prototypes', xpad, fpad, domains)
            loss = out[-2].square().sum() + (out[0].sum() if il else 0)
            loss.backward()
            res += [o.detach().clone() for o in out] + [m.flat.grad.clone()]
            res += [t.grad.clone() for t in (x, f) if t is not None and t.grad is not None]
            m.sgd_step(0.01)
            m.flat.grad.zero_()
        return res
    finally:
        T._LAYER_CALLS, T._DW_DEFER, ops.TIMER = old


def _add_temporal_cases():
    for mod in ("RGB", "Flow", "RGB-Flow"):
        for ns in (1, 2):
            for p in (0.0, 0.1):
                for lc, timer in ((True, False), (False, False), (False, True)):
                    kw = dict(mod=mod, ns=ns, p=p, layer_calls=lc, timer=timer)
                    case("train %s ns%d p%g layer_calls=%d timer=%d" % (mod, ns, p, lc, timer), real=True)(
                        lambda dev, kw=kw: _temporal(dev, **kw))
    extra = {"unequal streams": dict(Tx=9, Tf=2), "unequal streams launches": dict(Tx=9, Tf=2, layer_calls=False),
             "unequal streams ns2 padded": dict(Tx=9, Tf=2, ns=2, pads=True),
             "dw_defer off": dict(dw_defer=False), "dw_defer off p0": dict(dw_defer=False, p=0.0),
             "dw_defer off launches": dict(dw_defer=False, layer_calls=False),
             "importance head": dict(il=True), "importance head RGB launches": dict(il=True, mod="RGB", layer_calls=False),
             "multi-domain second": dict(domain="NH_02+X"), "multi-domain second ns2": dict(domain="NH_02+X", ns=2, p=0.0),
             "multi-domain RGB": dict(domain="NH_02+X", mod="RGB"),
             "hook": dict(hook=True), "hook launches": dict(hook=True, layer_calls=False),
             "x.requires_grad": dict(xgrad=True), "x.requires_grad launches ns2": dict(xgrad=True, layer_calls=False, ns=2),
             "x.requires_grad Flow": dict(xgrad=True, mod="Flow")}
    for name, kw in extra.items():
        case("train " + name, real=True)(lambda dev, kw=kw: _temporal(dev, **kw))


def _tta_inputs(dev, B=2, ns=1):
    import torch
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(B, ns, T, 384, generator=g).to(dev) for T in (15, 14, 13)]
    fs = [torch.randn(B, ns, T, 384, generator=g).to(dev) for T in (2, 1, 2)]
    xpads = [torch.zeros(B, ns, t.shape[2] + 1, dtype=torch.bool) for t in xs]
    fpads = [torch.zeros(B, ns, t.shape[2] + 1, dtype=torch.bool) for t in fs]
    fpads[0][0, :, -1] = True
    return xs, fs, xpads, fpads


def _tta(dev, mod="RGB-Flow", merge=True, train=False, il=False, domain="NH_02", grad=False, ns=1):
    import torch
    from sais_amd import temporal as T
    m = T.fullModel('reps', 2, domain, 384, 'ViT', modalities=mod, importance_loss=il).to(dev)
    m.train(train)
    old = T._TTA_MERGE
    T._TTA_MERGE = merge
    try:
        xs, fs, xpads, fpads = _tta_inputs(dev, ns=ns)
        domains = ["NH_02", "other"] if "+" in domain else None
        with torch.set_grad_enabled(grad):
            out = m(xs if mod != "Flow" else None, fs if mod != "RGB" else None, None, None, 'Prototypes', xpads, fpads, domains)
        flat = []
        for o in out:
            flat += [t.detach().clone() for t in (o if isinstance(o, (list, tuple)) else [o])]
        return flat
    finally:
        T._TTA_MERGE = old


def _add_inference_cases():
    for mod in ("RGB", "Flow", "RGB-Flow"):
        for merge in (True, False):
            case("tta list %s merge=%d" % (mod, merge), real=True)(lambda dev, mod=mod, merge=merge: _tta(dev, mod, merge))
    case("tta list ns2 merge=1", real=True)(lambda dev: _tta(dev, ns=2))
    case("tta list train() under no_grad", real=True)(lambda dev: _tta(dev, train=True))
    case("tta list train() under no_grad merge=0", real=True)(lambda dev: _tta(dev, train=True, merge=False))
    case("tta list with autograd (eval)", real=True)(lambda dev: _tta(dev, grad=True))
    case("tta list importance head", real=True)(lambda dev: _tta(dev, il=True))
    case("tta list multi-domain", real=True)(lambda dev: _tta(dev, domain="NH_02+X"))

    @case("task MIL", real=True)
    def _mil(dev):
        import torch
        from sais_amd import temporal as T
        m = T.fullModel('reps', 2, 'NH_02', 384, 'ViT').to(dev).eval()
        g = torch.Generator().manual_seed(7)
        x, f = torch.randn(2, 3, 8, 384, generator=g).to(dev), torch.randn(2, 3, 8, 384, generator=g).to(dev)
        seq, reps, logits, att = m(x, f, None, None, 'MIL', None, None)
        return [seq.clone(), reps, logits] + [att[c] for c in sorted(att)]

    def windows(dev, mod="RGB-Flow", il=False, domain="NH_02", merge=True, **kw):
        import torch
        from sais_amd import temporal as T
        from sais_amd.inference import run_windows
        m = T.fullModel('reps', 2, domain, 384, 'ViT', modalities=mod, importance_loss=il).to(dev)
        g = torch.Generator().manual_seed(9)
        rgb, flow = torch.randn(200, 384, generator=g).to(dev), torch.randn(14, 384, generator=g).to(dev)
        old = T._TTA_MERGE
        T._TTA_MERGE = merge
        try:
            r, attn, imp = run_windows(m, rgb, flow, videoname="v", batch_size=2, **kw)
        finally:
            T._TTA_MERGE = old
        return list(_tensors(r)) + list(attn) + list(imp)

    case("run_windows default", real=True)(lambda dev: windows(dev))
    case("run_windows merge=0", real=True)(lambda dev: windows(dev, merge=False))
    case("run_windows compute_batch=4", real=True)(lambda dev: windows(dev, compute_batch=4))
    case("run_windows Flow", real=True)(lambda dev: windows(dev, mod="Flow"))
    case("run_windows RGB", real=True)(lambda dev: windows(dev, mod="RGB"))
    case("run_windows importance_loss", real=True)(lambda dev: windows(dev, il=True))
    case("run_windows multi-domain RGB-Flow", real=True)(lambda dev: windows(dev, domain="NH_02+X"))
    case("run_windows multi-domain RGB", real=True)(lambda dev: windows(dev, domain="NH_02+X", mod="RGB"))


def _tensors(o):
    import torch
    if isinstance(o, torch.Tensor):
        yield o
    elif isinstance(o, dict):
        for k in sorted(o, key=str):
            yield from _tensors(o[k])
    elif isinstance(o, (list, tuple)):
        for v in o:
            yield from _tensors(v)


def _small_head():
    from sais_amd.dino import DINOHead
    return DINOHead(384, 256, hidden_dim=256, bottleneck_dim=128)


def _add_freshness_cases():
    @case("fresh vit")
    def _(dev):
        from sais_amd.vit import vit_small
        m = _engine_events(vit_small(depth=2), dev, None, "norm.weight")
        REC.log.append(["event", "sgd_step"])
        m.sgd_step(0.1)
        REC.log.append(["event", "after sgd_step"])
        m._engine(dev)

    @case("fresh temporal")
    def _(dev):
        from sais_amd.temporal import fullModel
        m = _engine_events(fullModel('reps', 2, 'NH_02', 384, 'ViT'), dev, None, "frame_cls")
        REC.log.append(["event", "sgd_step"])
        m.sgd_step(0.1)
        REC.log.append(["event", "after sgd_step"])
        m._engine(dev)

    @case("fresh DINOHead")
    def _(dev):
        _engine_events(_small_head(), dev, None, "mlp.4.bias")

    for teacher in (True, False):
        for frozen in (True, False):
            @case("DINOOptimizer.step teacher=%d frozen_last_layer=%d" % (teacher, frozen))
            def _(dev, teacher=teacher, frozen=frozen):
                from sais_amd.dino import DINOOptimizer, MultiCropWrapper
                from sais_amd.vit import vit_small
                nets = [MultiCropWrapper(vit_small(depth=2), _small_head()) for _ in range(2 if teacher else 1)]
                for n in nets:
                    n.backbone._engine(dev)
                    n.head._engine(dev)
                opt = DINOOptimizer(nets[0], nets[1] if teacher else None)
                for _ in range(2):
                    REC.log.append(["event", "step"])
                    opt.step(clip_grad=3.0, frozen_last_layer=frozen, ema_momentum=0.99 if teacher else None)
                    REC.log.append(["event", "engines after step"])
                    for n in nets:
                        n.backbone._engine(dev)
                        n.head._engine(dev)

    @case("trainModel broadcast branch")
    def _(dev):
        import torch
        import torch.distributed as dist
        from sais_amd import parallel, train
        from sais_amd.temporal import fullModel
        tm = fullModel('reps', 2, 'NH_02', 384, 'ViT')

        class Stop(Exception):
            pass

        class Sync:
            def __init__(self, world):
                pass

            def broadcast_initial_state(self, tensors):
                REC.log.append(["event", "broadcast", len(tensors)])
                tensors[0].mul_(0.5)

            def agree_max(self, t, device):
                return t

            def temporal_hook(self, model, tmax):
                raise Stop

        saved = train.loadModel, parallel.GradSync, dist.is_initialized
        train.loadModel = lambda *a, **k: ({"model": tm, "prototypes": {}}, None, dev)
        parallel.GradSync, dist.is_initialized = Sync, lambda: True
        try:
            train.trainModel(0, 2, "", "", "", 'reps', 2, 2, 'NH_02', ["train"], 0.1, 'RGB-Flow', True, False, 'Prototypes',
                             False, None, None, None, True, False, 'ViT', None, 1, 1, 0, 384, 1, 0, 1.0,
                             dataloader={"train": type("DL", (), {"dataset": []})()})
        except Stop:
            pass
        finally:
            train.loadModel, parallel.GradSync, dist.is_initialized = saved
        REC.log.append(["event", "engine after the broadcast"])
        tm._engine(dev)
        REC.log.append(["event", "engine again"])
        tm._engine(dev)


def _add_vit_cases():
    def vit(dev, frames, block_calls, train):
        import torch
        from sais_amd.vit import vit_small
        m = vit_small().to(dev)
        m.block_calls = block_calls
        m.train(train)
        m.grad_ready_hook = lambda lo, hi: REC.log.append(["hook", lo, hi])
        x = torch.zeros(frames, 3, 224, 224).to(dev)
        if train:
            m(x).sum().backward()
        else:
            with torch.no_grad():
                m(x)

    case("vit train 48 frames block_calls=1")(lambda dev: vit(dev, 48, True, True))
    case("vit train 48 frames block_calls=0")(lambda dev: vit(dev, 48, False, True))
    case("vit eval 6 frames")(lambda dev: vit(dev, 6, True, False))

    def frozen(dev, call, frames, H=224, W=224, depth=12):
        """One inference entry of the frozen backbone; 48 frames of 160 x 272 or of 224 x 224 are past the row-kernel dispatch."""
        import torch
        from sais_amd.vit import vit_small
        m = vit_small(depth=depth).to(dev).eval()
        with torch.no_grad():
            call(m, torch.zeros(frames, 3, H, W).to(dev))

    for name, frames, H, W, n in (("2 x 160x272 n=2", 2, 160, 272, 2), ("48 x 160x272 n=2", 48, 160, 272, 2),
                                  ("2 x 224x224 n=1", 2, 224, 224, 1), ("2 x 208x336 n=2", 2, 208, 336, 2)):
        case("vit dense_features " + name)(lambda dev, a=(frames, H, W), n=n: frozen(dev, lambda m, x: m.dense_features(x, n), *a))
    for name, frames, H, W, depth in (("2 x 64x96", 2, 64, 96, 12), ("48 x 224x224", 48, 224, 224, 12),
                                      ("2 x 64x96 depth=1", 2, 64, 96, 1)):
        case("vit cls_attention " + name)(lambda dev, a=(frames, H, W, depth): frozen(dev, lambda m, x: m.cls_attention(x), *a))
    for frames in (2, 48):
        case("vit get_intermediate_layers n=2 %d frames" % frames)(
            lambda dev, frames=frames: frozen(dev, lambda m, x: m.get_intermediate_layers(x, 2), frames))
    case("vit probe_features n=4 2 frames")(lambda dev: frozen(dev, lambda m, x: m.probe_features(x, 4), 2))
    case("vit probe_features avgpool 2 frames")(lambda dev: frozen(dev, lambda m, x: m.probe_features(x, 1, avgpool=True), 2))
    for side in (224, 96):
        case("vit get_last_selfattention 2 x %dx%d" % (side, side))(
            lambda dev, side=side: frozen(dev, lambda m, x: m.get_last_selfattention(x), 2, side, side))

    @case("vit two resolutions, no save")
    def _(dev):
        import torch
        from sais_amd.vit import vit_small
        m = vit_small().to(dev).eval()
        m._engine(dev)
        with torch.no_grad():
            m._forward_kernels([torch.zeros(2, 3, 224, 224).to(dev), torch.zeros(3, 3, 96, 96).to(dev)], save=False)


def _add_vit_form_cases():
    """The three forms of a ViT pass (resident, streaming, segmented) in both directions, patch 8, the retrieval tails and the
    combinations the package refuses.  depth = 2 unless a case needs more."""
    import torch
    from sais_amd import ops
    from sais_amd.vit import vit_small
    MIXED = ((1, 224, 224), (2, 64, 96), (1, 160, 272))

    def model(dev, train=False, dpr=0.0, depth=2, patch=16, **attrs):
        m = vit_small(patch_size=patch, depth=depth, drop_path_rate=dpr).to(dev)
        m.train(train)
        m.grad_ready_hook = lambda lo, hi: REC.log.append(["hook", lo, hi])
        for k, v in attrs.items():
            setattr(m, k, v)
        return m

    def frames(dev, *shapes):
        return [torch.zeros(n, 3, H, W).to(dev) for n, H, W in shapes]

    def saved_pass(dev, shapes, seg=False, timer=False, **kw):
        """_forward_kernels(save=True) + _backward_kernels on resolution groups, or on the frames as segments."""
        m, x = model(dev, **kw), frames(dev, *shapes)
        m._engine(dev)
        old = ops.TIMER
        if timer:
            ops.TIMER = ops.KernelTimer()
        try:
            reps, saved = m._forward_kernels(x, save=True, streaming=True if seg else m.streaming_pass(x),
                                             seg=m._seg_plan(x) if seg else None)
            m._backward_kernels(saved, torch.ones_like(reps))
        finally:
            ops.TIMER = old

    def train_step(dev, x, timer=False, **kw):
        m, old = model(dev, **kw), ops.TIMER
        if timer:
            ops.TIMER = ops.KernelTimer()
        try:
            m(x).sum().backward()
        finally:
            ops.TIMER = old

    for tag, kw in (("", {}), (" droppath", dict(train=True, dpr=0.1))):
        case("vit streaming train 2 x 64x96" + tag)(lambda dev, kw=kw: train_step(dev, frames(dev, (2, 64, 96))[0], **kw))
        case("vit streaming train 1 x 224x240" + tag)(lambda dev, kw=kw: train_step(dev, frames(dev, (1, 224, 240))[0], **kw))
        case("vit streaming saved list pass" + tag)(lambda dev, kw=kw: saved_pass(dev, ((2, 224, 224), (3, 96, 128)), **kw))
        for prune in (True, False):
            for name, shapes in (("2x224 3x96", ((2, 224, 224), (3, 96, 96))), ("48x224 256x96", ((48, 224, 224), (256, 96, 96)))):
                case("vit resident saved list pass %s prune=%d%s" % (name, prune, tag))(
                    lambda dev, kw=kw, shapes=shapes, prune=prune: saved_pass(dev, shapes, prune_last_block=prune, **kw))
        case("vit segmented train" + tag)(lambda dev, kw=kw: train_step(dev, frames(dev, *MIXED), **kw))
        case("vit segmented train timer" + tag)(lambda dev, kw=kw: train_step(dev, frames(dev, *MIXED), timer=True, **kw))
        case("vit segmented train 48 x 224x224" + tag)(lambda dev, kw=kw: train_step(dev, frames(dev, (48, 224, 224)), **kw))
        case("vit segmented saved pass" + tag)(lambda dev, kw=kw: saved_pass(dev, MIXED, seg=True, **kw))

    def frozen(dev, call, shapes=MIXED, depth=2, patch=16):
        m = model(dev, depth=depth, patch=patch)
        with torch.no_grad():
            call(m, frames(dev, *shapes))

    case("vit segmented dense_features n=2")(lambda dev: frozen(dev, lambda m, x: m.dense_features(x, 2)))
    case("vit segmented retrieval_features cls_only")(lambda dev: frozen(dev, lambda m, x: m.retrieval_features(x, cls_only=True)))
    case("vit segmented forward no_grad")(lambda dev: frozen(dev, lambda m, x: m(x)))
    case("vit segmented forward no_grad 48 x 224x224")(lambda dev: frozen(dev, lambda m, x: m(x), ((48, 224, 224),)))
    for cls_only in (False, True):
        case("vit retrieval_features 2 x 160x272 cls_only=%d" % cls_only)(
            lambda dev, c=cls_only: frozen(dev, lambda m, x: m.retrieval_features(x[0], cls_only=c), ((2, 160, 272),)))
        case("vit8 retrieval_features 2 x 64x96 cls_only=%d" % cls_only)(
            lambda dev, c=cls_only: frozen(dev, lambda m, x: m.retrieval_features(x[0], cls_only=c), ((2, 64, 96),), patch=8))
    for name, call, shapes, depth in (
            ("forward 2 x 224x224", lambda m, x: m(x[0]), ((2, 224, 224),), 2),
            ("forward 2 x 64x96", lambda m, x: m(x[0]), ((2, 64, 96),), 2),
            ("dense_features n=2", lambda m, x: m.dense_features(x[0], 2), ((2, 64, 96),), 2),
            ("get_intermediate_layers n=2", lambda m, x: m.get_intermediate_layers(x[0], 2), ((2, 64, 96),), 2),
            ("probe_features n=4", lambda m, x: m.probe_features(x[0], 4), ((2, 64, 96),), 4),
            ("probe_features avgpool", lambda m, x: m.probe_features(x[0], 1, avgpool=True), ((2, 64, 96),), 2),
            ("cls_attention", lambda m, x: m.cls_attention(x[0]), ((2, 64, 96),), 2)):
        case("vit8 " + name)(lambda dev, a=(call, shapes, depth): frozen(dev, *a, patch=8))

    def multicrop(dev, segmented):
        from sais_amd.dino import MultiCropWrapper
        old = os.environ.pop("SAIS_DINO_SEGMENTED", None)
        if segmented:
            os.environ["SAIS_DINO_SEGMENTED"] = "1"
        try:
            w = MultiCropWrapper(model(dev), _small_head())
        finally:
            os.environ.pop("SAIS_DINO_SEGMENTED", None)
            if old is not None:
                os.environ["SAIS_DINO_SEGMENTED"] = old
        w.head._engine(dev)
        logits, saved = w.forward_kernels(frames(dev, *([(2, 224, 224)] * 2 + [(2, 96, 96)] * 3)), save=True)
        w.backward_kernels(saved, torch.zeros_like(logits))

    case("MultiCropWrapper 2 global + 3 local crops")(lambda dev: multicrop(dev, False))
    case("MultiCropWrapper 2 global + 3 local crops SAIS_DINO_SEGMENTED=1")(lambda dev: multicrop(dev, True))

    def refused(dev, call, shapes=((1, 32, 48),), patch=16, grad=False):
        m = model(dev, patch=patch)
        m._engine(dev)
        with torch.set_grad_enabled(grad):
            call(m, frames(dev, *shapes))

    for name, end in (("streaming=False", "reps"), ("end=probs", "probs"), ("end=norm1", "norm1")):
        case("vit refuses seg with " + name)(lambda dev, end=end, s=name != "streaming=False": refused(
            dev, lambda m, x: m._forward_kernels(x, save=False, end=end, streaming=s, seg=m._seg_plan(x))))
    case("vit refuses seg of other rows")(lambda dev: refused(
        dev, lambda m, x: m._forward_kernels(x, save=False, streaming=True, seg=m._seg_plan(x[:1])), ((1, 32, 48), (1, 64, 64))))
    case("vit8 refuses a list: dense_features")(lambda dev: refused(dev, lambda m, x: m.dense_features(x), patch=8))
    case("vit8 refuses a list: forward")(lambda dev: refused(dev, lambda m, x: m(x), patch=8))
    case("vit8 refuses forward under grad")(lambda dev: refused(dev, lambda m, x: m(x[0]), patch=8, grad=True))
    case("vit refuses an empty list")(lambda dev: refused(dev, lambda m, x: m([])))
    case("vit refuses retrieval_features(list) without cls_only")(lambda dev: refused(dev, lambda m, x: m.retrieval_features(x)))
    case("vit refuses probs of two groups")(lambda dev: refused(
        dev, lambda m, x: m._forward_kernels(x, save=False, end="probs"), ((1, 224, 224), (1, 96, 96))))


# ------------------------------------------------------------------------------------------------ driver
def run(root, out, real):
    sys.path.insert(0, os.path.abspath(root))
    import torch
    if not real:
        install_recorder()
    _add_temporal_cases()
    _add_inference_cases()
    _add_freshness_cases()
    _add_vit_cases()
    _add_vit_form_cases()
    dev = torch.device("cuda:0" if real else "cpu")
    logs, results = {}, {}
    for i, (name, fn, in_real) in enumerate(CASES):
        if real and not in_real:
            continue
        REC.reset()
        torch.manual_seed(100 + i)
        try:
            res = fn(dev)
        except (ValueError, NotImplementedError) as e:                 # a case the package refuses: the refusal is the record
            REC.log.append(["raises", type(e).__name__, str(e)])
            res = None
        logs[name] = REC.log
        if real:
            torch.cuda.synchronize()
            results[name] = [_pack(t) for t in _tensors(res)] if res is not None else REC.log
        print("%-60s %5d entries" % (name, len(REC.log)), flush=True)
    REC.reset()
    if real:
        torch.save(results, out)
    else:
        with open(out, "w") as fh:
            json.dump(logs, fh)


def _pack(t, full=1 << 21):
    """A result tensor for the .pt file: itself, or (a flat gradient buffer of 19 M elements per case) its sha256 and every 31st
    element; bit-equality is then decided by the hash and the largest difference is that of the sample."""
    import hashlib
    t = t.detach().cpu().contiguous()
    if t.numel() <= full:
        return t
    return dict(sha256=hashlib.sha256(t.numpy().tobytes()).hexdigest(), sample=t.reshape(-1)[::31].clone())


def compare(a, b, out):
    rows, bad = {}, 0
    if a.endswith(".pt"):
        import torch
        A, B = torch.load(a), torch.load(b)
        for name in A:
            if name not in B or len(A[name]) != len(B[name]):
                rows[name], bad = "MISSING or different length", bad + 1
                continue
            if A[name] and not isinstance(A[name][0], torch.Tensor):
                rows[name] = "refused alike" if A[name] == B[name] else "DIFFERENT refusal"
                continue
            same, worst = True, 0.0
            for x, y in zip(A[name], B[name]):
                if isinstance(x, dict):
                    same, x, y = same and x["sha256"] == y["sha256"], x["sample"], y["sample"]
                same = same and x.shape == y.shape and torch.equal(x, y)
                if x.shape == y.shape and x.numel():
                    worst = max(worst, float((x.double() - y.double()).abs().max()))
            rows[name] = dict(bit_equal=same, max_abs_diff=worst, tensors=len(A[name]))
    else:
        A, B = json.load(open(a)), json.load(open(b))
        for name in sorted(set(A) | set(B)):
            la, lb = A.get(name), B.get(name)
            first = None
            if la != lb:
                bad += 1
                n = min(len(la or []), len(lb or []))
                first = next((i for i in range(n) if la[i] != lb[i]), n)
            rows[name] = dict(entries=len(la or []), equal=la == lb, first_difference=first)
            if first is not None:
                print("DIFFERENT %s at entry %d:\n  %s\n  %s" % (name, first, (la or [None] * (first + 1))[first:first + 1],
                                                                  (lb or [None] * (first + 1))[first:first + 1]))
    summary = dict(a=os.path.basename(a), b=os.path.basename(b), cases=len(rows), different=bad, rows=rows)
    print(json.dumps({k: v for k, v in summary.items() if k != "rows"}))
    if out:
        with open(out, "w") as fh:
            json.dump(summary, fh, indent=1)
    return bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out")
    ap.add_argument("--real", action="store_true")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.compare:
        sys.exit(1 if compare(a.compare[0], a.compare[1], a.json) else 0)
    run(a.root, a.out, a.real)
