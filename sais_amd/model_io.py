"""Checkpoint codec + model factory — drop-in for `loadModel` (SAIS/scripts/prepare_model.py:517-570)
and the save step of `trainModel` (train.py:98-121).  File contracts:

  params.zip      torch.save(state_dict of fullModel) with EVERY key prefixed `module.` (DDP era); may carry
                  `encoder.*` tensors of the unused timm ViT-B (ignored here, never instantiated)
  prototypes.zip  torch.save(nn.ParameterDict{'0': Parameter[1,256], ...})  — a pickled module object,
                  so torch >= 2.6 needs weights_only=False
  dino_deitsmall16_pretrain.pth   plain state_dict of vit_small, 150 tensors, loaded strict
  checkpoint.pth  of main_dino.py: {'student': ..., 'teacher': ..., ...} with `module.` / `backbone.` prefixes — the frozen
                  backbone of the DINO tools (eval_knn.py, eval_linear.py, eval_video_segmentation.py, the attention-map scripts)
"""
import argparse
import os

import torch
import torch.nn as nn

from .optim import SGD
from .temporal import fullModel
from .vit import vit_small


def strip_module_prefix(params):
    """prepare_model.py:524-527: `name.split('module.')[1]`; a key without the prefix raises (IndexError there)."""
    out = {}
    for name, t in params.items():
        parts = name.split('module.')
        if len(parts) < 2:
            raise IndexError(f"checkpoint key {name!r} lacks the 'module.' prefix (prepare_model.py:526)")
        out[parts[1]] = t
    return out


def load_params_file(path):
    params = torch.load(path, map_location='cpu', weights_only=False)
    params = strip_module_prefix(params)
    return {k: v for k, v in params.items() if not k.startswith('encoder.')}     # timm ViT-B ballast, unused


def save_params_file(model, path):
    """What train.py:108 writes as `params` (README renames to params.zip): module.-prefixed state_dict."""
    sd = {'module.' + k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    torch.save(sd, path)


def save_prototypes_file(prototypes, path):
    pd = nn.ParameterDict()
    for k in prototypes.keys():
        pd[k] = nn.Parameter(prototypes[k].detach().cpu().clone())
    torch.save(pd, path)


def load_prototypes_file(path, device):
    protos = torch.load(path, map_location='cpu', weights_only=False)
    out = nn.ParameterDict()
    for k in protos.keys():
        out[k] = nn.Parameter(protos[k].detach().clone().to(device))
    return out


def loadModel(rank, world_size, savepath, data_type, nclasses, domain, rep_dim, encoder_type, task, fold, lr=0.001,
              modalities='RGB-Flow', freeze_encoder_params=True, self_attention=True, importance_loss=False,
              inference=False, device=None):
    """Same positional signature and return value as the reference: ({'model','prototypes'}, optimizer, device).
    The reference pins device='cpu' (:544); here the model lives on the rank's MI355X."""
    device = torch.device(device if device is not None else f"cuda:{rank}")
    model = fullModel(data_type, nclasses, domain, rep_dim, encoder_type, modalities=modalities,
                      freeze_encoder_params=freeze_encoder_params, self_attention=self_attention,
                      importance_loss=importance_loss)
    if inference:
        new_params = load_params_file(os.path.join(savepath, 'params.zip'))
        print('# of Loaded Params: %i' % len(new_params), '# of Model Params: %i' % len(dict(model.named_parameters())))
        model.load_state_dict(new_params)                       # strict, as :529
        print('Params Loaded...')
    model.to(device)
    if not inference:
        protos = nn.ParameterDict()
        for c in range(nclasses):
            protos[str(c)] = nn.Parameter(torch.rand(1, 256, device=device))     # :556-560
    else:
        protos = load_prototypes_file(os.path.join(savepath, 'prototypes.zip'), device)
        print('Prototypes Loaded!')
    params = list(model.parameters()) + list(protos.values())
    optimizer = SGD(params, lr=lr, engines=[model])
    return {'model': model, 'prototypes': protos}, optimizer, device


def load_vit(path=None, device='cuda:0', drop_path_rate=0.1, patch_size=16):
    """extract_representations.loadModel (:181-219): vit_small(patch_size) + strict load of the DINO checkpoint (patch 16:
    dino_deitsmall16_pretrain.pth; patch 8, inference only: dino_deitsmall8_pretrain.pth)."""
    model = vit_small(patch_size=patch_size, drop_path_rate=drop_path_rate)
    if path is not None:
        sd = torch.load(path, map_location='cpu', weights_only=False)
        if isinstance(sd, dict) and 'student' in sd:            # surgical-DINO variant (:190-199)
            items = list(sd['student'].items())[:-8]
            sd = {'.'.join(k.split('.')[2:]): v for k, v in items}
        model.load_state_dict(sd, strict=True)
    return model.to(device).eval()


def backbone_state_dict(ckpt, checkpoint_key="teacher"):
    """utils.load_pretrained_weights (utils.py:55-65): take `checkpoint_key` when the file has it, strip the `module.` and
    `backbone.` prefixes.  A bare backbone state_dict passes through."""
    sd = ckpt
    if checkpoint_key is not None and isinstance(ckpt, dict) and checkpoint_key in ckpt:
        sd = ckpt[checkpoint_key]
    sd = {k.replace("module.", ""): v for k, v in sd.items()}
    return {k.replace("backbone.", ""): v for k, v in sd.items()}


def load_dino_backbone(args, dev, seed=None, freeze=False, random="random"):
    """The frozen backbone of a DINO tool from its parsed flags (--arch, --patch_size, --pretrained_weights,
    --checkpoint_key): vit_small with 16 x 16 or 8 x 8 patches in eval(), with the checkpoint loaded as utils.load_pretrained_weights does, else the
    weights of its initialisation and a message; never a download.  seed: torch's seed before the initialisation (a backbone
    without --pretrained_weights is then the same in every invocation); freeze: no parameter requires a gradient; random:
    how the message names the weights that stay."""
    if args.arch.replace("deit", "vit") != "vit_small" or args.patch_size not in (16, 8):
        raise NotImplementedError("MI355X path: --arch vit_small --patch_size 16 (or --patch_size 8, inference only)")
    if seed is not None:
        torch.manual_seed(seed)
    model = vit_small(patch_size=args.patch_size, num_classes=0).to(dev)
    if args.pretrained_weights and os.path.isfile(args.pretrained_weights):
        ckpt = torch.load(args.pretrained_weights, map_location="cpu", weights_only=False)
        if args.checkpoint_key is not None and isinstance(ckpt, dict) and args.checkpoint_key in ckpt:
            print(f"Take key {args.checkpoint_key} in provided checkpoint dict")
        msg = model.load_state_dict(backbone_state_dict(ckpt, args.checkpoint_key), strict=False)
        print('Pretrained weights found at {} and loaded with msg: {}'.format(args.pretrained_weights, msg))
    else:
        print("Please use the `--pretrained_weights` argument to indicate the path of the checkpoint to evaluate.")
        print(f"There is no reference to load pretrained weights from: the model keeps its {random} weights.")
    if freeze:
        for p in model.parameters():
            p.requires_grad = False
    return model.eval()


def bool_flag(s):
    """utils.bool_flag (utils.py:201-212), the argparse type of the DINO tools' on / off flags."""
    if s.lower() in {"off", "false", "0"}:
        return False
    if s.lower() in {"on", "true", "1"}:
        return True
    raise argparse.ArgumentTypeError("invalid value for a boolean flag")
