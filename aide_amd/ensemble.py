"""Test-time augmentation: the eight flips and quarter turns of an image, and the soft vote over them.

A view code is `v = r + 4 * f` (r = 0 .. 3 quarter turns, f = 0 / 1 a flip of the last axis first):

    view_v(x) = torch.rot90(torch.flip(x, [-1]) if f else x, r, (-2, -1))

The views are exact permutations of the pixels: nothing is interpolated.  A member of an ensemble is a network's logits
for one view, left in that view's frame; the vote reads every member through the inverse of its view, takes the fp32
soft-max, adds the members IN ORDER, multiplies by 1 / K and labels a pixel with the FIRST class of the largest sum
(`aide_ensemble_vote`, csrc/ensemble.hip; `ensemble_vote_host` is the same order of fp32 operations in torch).  The views of
a batch are made by one launch (`aide_view_stack`) and go through the network as ONE batch: eval-mode BatchNorm uses the
running statistics, so the slices of a batch are independent.
"""
import ctypes

import torch

from ._lib import lib, check
from .ops import ptr, stream_ptr

VIEW_SETS = {
    'flip2': (0, 4),                       # identity and the left-right flip
    'flip4': (0, 4, 2, 6),                 # ... and their half turns: the four views of a rectangle
    'd4': (0, 1, 2, 3, 4, 5, 6, 7),        # the symmetries of a square
}
MAX_MEMBERS = 16
MAX_CLASSES = 8                            # aide_seg_max_classes()


def view_codes(views, h=None, w=None):
    """A named set ('flip2', 'flip4', 'd4') or a sequence of codes -> tuple of ints, checked: ValueError for an unknown name,
    an empty set, a code outside 0 .. 7, or (h, w given) a quarter turn of an image that is not square."""
    if isinstance(views, str):
        if views not in VIEW_SETS:
            raise ValueError('unknown view set %r: one of %s or a tuple of codes r + 4 * f' % (views, sorted(VIEW_SETS)))
        codes = VIEW_SETS[views]
    else:
        try:
            codes = tuple(views)
        except TypeError:
            raise ValueError('views: a set name or a sequence of view codes expected, got %r' % (views,))
    if not codes:
        raise ValueError('views: at least one view code')
    for v in codes:
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 7:
            raise ValueError('view code %r: an int 0 .. 7 (r + 4 * f) expected' % (v,))
        if v & 1 and h is not None and h != w:
            raise ValueError('view code %d is a quarter turn: the image must be square, got %d x %d' % (v, h, w))
    return tuple(codes)


def view_apply_host(x, code):
    """view_code(x) of a [..., H, W] tensor: the definition, in torch."""
    (code,) = view_codes((code,), *x.shape[-2:])
    return torch.rot90(torch.flip(x, [-1]) if code & 4 else x, code & 3, (-2, -1))


def view_invert_host(y, code):
    """The inverse: view_invert_host(view_apply_host(x, code), code) == x."""
    (code,) = view_codes((code,), *y.shape[-2:])
    x = torch.rot90(y, -(code & 3), (-2, -1))
    return torch.flip(x, [-1]) if code & 4 else x


def _members(member_logits, views):
    zs = list(member_logits)
    if not zs:
        raise ValueError('ensemble_vote: at least one member')
    if len(zs) > MAX_MEMBERS:
        raise ValueError('ensemble_vote: %d members, at most %d' % (len(zs), MAX_MEMBERS))
    z0 = zs[0]
    if z0.dim() != 4 or not 2 <= z0.shape[1] <= MAX_CLASSES:
        raise ValueError('ensemble_vote: members are [N,C,H,W] logits with 2 <= C <= %d' % MAX_CLASSES)
    if any(z.shape != z0.shape or z.dtype != torch.float32 or z.device != z0.device for z in zs):
        raise ValueError('ensemble_vote: the members must be fp32 tensors of one shape on one device')
    n, c, h, w = z0.shape
    codes = view_codes(views, h, w)
    if len(codes) != len(zs):
        raise ValueError('ensemble_vote: %d members but %d view codes' % (len(zs), len(codes)))
    if n * c * h * w >= 2 ** 31:
        raise ValueError('ensemble_vote: %d logits per member, fewer than 2^31 expected' % (n * c * h * w))
    return zs, codes


def ensemble_vote_host(member_logits, views, probs=False):
    """The host statement of `aide_ensemble_vote` in torch, operation for operation in fp32: per member (in order) the inverse
    view, m = max_c z, e_c = exp(z_c - m), s = e_0 + e_1 + ..., p_c = e_c * (1 / s); sum_c += p_c; probs = sum * fp32(1 / K);
    label = the first class of the largest sum."""
    zs, codes = _members(member_logits, views)
    c = zs[0].shape[1]
    acc = None
    for z, v in zip(zs, codes):
        z = view_invert_host(z.detach(), v)
        e = torch.exp(z - z.max(1, keepdim=True).values)
        s = e[:, 0:1]
        for k in range(1, c):
            s = s + e[:, k:k + 1]
        p = e * (1.0 / s)
        acc = p if acc is None else acc + p
    best = acc[:, 0]
    labels = torch.zeros(best.shape, dtype=torch.int64, device=acc.device)
    for k in range(1, c):
        gt = acc[:, k] > best
        best = torch.where(gt, acc[:, k], best)
        labels[gt] = k
    if not probs:
        return labels
    return labels, acc * torch.tensor(1.0 / len(zs), dtype=torch.float32, device=acc.device)


def ensemble_vote(member_logits, views, probs=False):
    """K members' logits (a sequence of [N,C,H,W] fp32 tensors, member k in the frame of view views[k]; K <= 16, C = 2 .. 8)
    -> int64 labels [N,H,W] in the input frame, with probs=True also the mean soft-max fp32 [N,C,H,W].  HIP tensors: one
    launch of `aide_ensemble_vote`, no copy of any member (a slice of a stacked batch is a member as it stands); CPU
    tensors: `ensemble_vote_host`.  One member under view 0 gives `label_map`'s labels."""
    zs, codes = _members(member_logits, views)
    if not zs[0].is_cuda:
        return ensemble_vote_host(zs, codes, probs)
    zs = [z.detach() if z.is_contiguous() else z.detach().contiguous() for z in zs]
    n, c, h, w = zs[0].shape
    labels = torch.empty(n, h, w, device=zs[0].device, dtype=torch.int64)
    pr = torch.empty(n, c, h, w, device=zs[0].device, dtype=torch.float32) if probs else None
    arr = (ctypes.c_void_p * len(zs))(*[z.data_ptr() for z in zs])
    va = (ctypes.c_int * len(zs))(*codes)
    check(lib.aide_ensemble_vote(arr, va, len(zs), c * h * w, n, c, h, w, ptr(labels), ptr(pr), c * h * w, stream_ptr()),
          'ensemble_vote')
    return (labels, pr) if probs else labels


def view_stack(x, views):
    """[N,C,H,W] fp32 -> [V,N,C,H,W]: plane v is view_views[v](x).  HIP tensors: one launch of `aide_view_stack`, x read
    once; CPU tensors: torch.stack of `view_apply_host`."""
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError('view_stack: a [N,C,H,W] fp32 tensor expected')
    n, c, h, w = x.shape
    codes = view_codes(views, h, w)
    if len(codes) > MAX_MEMBERS:
        raise ValueError('view_stack: %d views, at most %d' % (len(codes), MAX_MEMBERS))
    if not x.is_cuda:
        return torch.stack([view_apply_host(x, v) for v in codes])
    if n * c * h * w >= 2 ** 31:
        raise ValueError('view_stack: %d elements, fewer than 2^31 expected' % (n * c * h * w))
    x = x.detach()
    if not x.is_contiguous():
        x = x.contiguous()
    y = torch.empty(len(codes), n, c, h, w, device=x.device, dtype=torch.float32)
    if x.numel():
        va = (ctypes.c_int * len(codes))(*codes)
        check(lib.aide_view_stack(ptr(x), c * h * w, ptr(y), c * h * w, va, len(codes), n, c, h, w, stream_ptr()), 'view_stack')
    return y


def _net_list(nets):
    nets = list(nets) if isinstance(nets, (list, tuple)) else [nets]
    if not nets:
        raise ValueError('ensemble: at least one network')
    for net in nets:
        if net.training:
            raise RuntimeError('predict_labels needs net.eval(): train-mode BatchNorm at bs=1 is not what the '
                               'reference loop runs')
    return nets


def _member_count(nets, codes):
    if len(nets) * len(codes) > MAX_MEMBERS:
        raise ValueError('ensemble: %d networks x %d views = %d members, at most %d'
                         % (len(nets), len(codes), len(nets) * len(codes), MAX_MEMBERS))


def member_logits(nets, modal_inputs, views):
    """-> (per network a [V,N,C,H,W] tensor of its logits in view frames, the member codes [len(nets) * V]).  One view stack
    per modality, one forward per network on the V * N stacked batch; nothing is copied afterwards."""
    nets = _net_list(nets)
    if not modal_inputs:
        raise TypeError('ensemble: no input')
    h, w = modal_inputs[0].shape[-2:]
    codes = view_codes(views, h, w)
    _member_count(nets, codes)
    with torch.no_grad():
        stacked = [view_stack(m, codes) for m in modal_inputs]
        stacked = [s.reshape((-1,) + tuple(s.shape[2:])) for s in stacked]
        outs = []
        for net in nets:
            z = net(*stacked).detach()
            if z.dim() != 4 or z.shape[0] != stacked[0].shape[0] or tuple(z.shape[-2:]) != (h, w):
                raise RuntimeError('ensemble: the network returned %s for a batch of %s' % (tuple(z.shape), tuple(stacked[0].shape)))
            if outs and z.shape[1] != outs[0].shape[2]:
                raise ValueError('ensemble: the networks differ in class count (%d and %d)' % (outs[0].shape[2], z.shape[1]))
            if not z.is_contiguous():
                z = z.contiguous()
            outs.append(z.view((len(codes), -1) + tuple(z.shape[1:])))
    return outs, codes * len(nets)


def ensemble_logits(nets, *modal_inputs, **kw):
    """Logits [K,N,C,H,W] of K = len(nets) * V members, member i * V + j = network i under view j, each in its view's frame:
    what `ensemble_vote(list(result), codes)` takes.  `nets`: a network or a list / tuple of them (eval mode); `modal_inputs`
    = (inphase[, outphase]) each [N,3,H,W]; views: a set name or codes.  One network: a view of its output batch; several:
    their outputs concatenated once (`predict_labels` hands the vote the per-network slices instead, without that copy)."""
    views = kw.pop('views')
    if kw:
        raise TypeError('unexpected arguments %r' % sorted(kw))
    outs, _ = member_logits(nets, modal_inputs, views)
    return outs[0] if len(outs) == 1 else torch.cat(outs, 0)


def predict_ensemble(nets, modal_inputs, views, batch_size=16, probs=False):
    """`predict_labels(..., views=...)`: int64 labels [S,H,W] (and the mean probabilities [S,C,H,W]) of S slices, voted over
    len(nets) * V members; max(1, batch_size // V) slices per forward, so a forward batch holds at most batch_size images
    (V of them when batch_size < V)."""
    nets = _net_list(nets)
    h, w = modal_inputs[0].shape[-2:]
    codes = view_codes(views, h, w)
    _member_count(nets, codes)
    s = modal_inputs[0].shape[0]
    dev = next(nets[0].parameters()).device
    step = max(1, int(batch_size) // len(codes))
    labels, pr = [], []
    for i in range(0, s, step):
        xs = [m[i:i + step].to(dev, non_blocking=True) for m in modal_inputs]
        outs, member_codes = member_logits(nets, xs, codes)
        r = ensemble_vote([o[j] for o in outs for j in range(len(codes))], member_codes, probs=probs)
        labels.append(r[0] if probs else r)
        if probs:
            pr.append(r[1])
    labels = torch.cat(labels, 0) if len(labels) > 1 else labels[0]
    if not probs:
        return labels
    return labels, (torch.cat(pr, 0) if len(pr) > 1 else pr[0])
