"""Training batches made on the device: what basicsr/data/continuous_bicubic_downsample_dataset.py:46-111 (and its `_sa1b`
variant) does per sample on the host -- float crop, bicubic LR (`imresize_new(crop, 1 / scale_modify)`), the shared flip /
transposition of basicsr/data/transforms.py:119-133, BGR -> RGB, HWC -> CHW, zero padding to `gt_size_max` or `sample_size`
picked pixels -- and the DataLoader's collation, as one call on decoded uint8 images.

    args, scales = draw_batch(image_sizes, lr_size, scale_list, rng)      host only: the dataset's random draws, in its order
    batch = make_batch(images, lr_size=lr_size, **args)                   {'gt', 'lq', 'gt_size', 'scale_modify', 'pad_h', 'pad_w'}

CUDA tensors: gsasr_batch_make / gsasr_batch_pick (hand-written HIP, csrc/splat_data.hip) on the current stream, no fallback.
CPU tensors: the same values from torch ops and `resize.resize_torch`, the executable statement of the contract in
include/gsasr_splat.h.

Left to the caller: decoding the images, `color: 'y'`, mean / std normalisation, and drawing `sample_coords`.
"""
import math

import torch

from .resize import _check_axis, resize_torch

__all__ = ["make_batch", "draw_batch"]

MAX_BATCH = 64      # GSASR_MAX_BATCH
MAX_SIDE = 32767


def _flags(v, B, name):
    if v is None:
        return [False] * B
    v = v.tolist() if torch.is_tensor(v) else list(v)
    if len(v) != B:
        raise ValueError(f"one {name} per sample")
    return [bool(x) for x in v]


def _augment(t, h, v, r):
    """transforms.py:119-133 on `[..., rows, cols]`: horizontal flip, then vertical flip, then transposition"""
    if h:
        t = t.flip(-1)
    if v:
        t = t.flip(-2)
    if r:
        t = t.transpose(-1, -2)
    return t


def make_batch(images, crops, lr_size, hflip=None, vflip=None, rot90=None, gt_pad=None, sample_coords=None, bgr=True, antialiasing=True):
    """The collated training batch of B crops, one call.

    `images`: a sequence of B uint8 tensors `[h_i, w_i, 3]`, contiguous, on one device (the same tensor may appear more than
    once); `crops`: B host tuples `(y0, x0, gh, gw)`; `lr_size`: an int or `(lh, lw)`; `hflip`, `vflip`, `rot90`: B booleans
    each (default none), applied in that order to GT and LR alike -- `rot90` is the reference's transposition, and needs a
    square crop and a square `lr_size`; `gt_pad`: `(Gh, Gw)`, the reference's `gt_size_max` (default: the largest sample --
    what `generate_2D_gaussian_splatting_batch_loss(targets=...)` reads in place); `bgr`: the bytes of a pixel are b, g, r (an
    image decoded by OpenCV) and the planes come out r, g, b.

    Returns a dict: `gt` `[B,3,Gh,Gw]` float32 (`byte / 255`, every pixel outside a sample exactly 0), `lq` `[B,3,lh,lw]`
    (`imresize_batch` of the un-augmented crops to `lr_size`, then augmented: the reference's order), `gt_size` CPU int64
    `[B,2]`, `scale_modify` CPU float32 `[B,2]` = `gh / lh`, `gw / lw`, `pad_h`, `pad_w` CPU int64 `[B]`.  With
    `sample_coords` (`[B,S,2]` integer (row, column) points of the augmented crop, on the images' device; a negative index wraps
    once, a point still out of range yields 0) `gt` is `[B,3,S]` -- the float GT image is not made --, the pad keys are absent
    and `sample_coords` is passed through.

    ValueError on anything else, including a crop whose resize breaks the reflection condition of `imresize`.  Not done here:
    image decoding, `color: 'y'`, mean / std normalisation, and drawing `sample_coords`."""
    if isinstance(images, torch.Tensor) or not hasattr(images, "__len__"):
        raise ValueError("images must be a sequence of uint8 tensors [h,w,3]")
    images = list(images)
    B = len(images)
    if not (1 <= B <= MAX_BATCH):
        raise ValueError(f"the batch must hold 1..{MAX_BATCH} samples")
    hw = []
    for t in images:
        sh = t.shape if torch.is_tensor(t) else ()
        if not (len(sh) == 3 and sh[2] == 3 and t.dtype == torch.uint8 and t.is_contiguous()):
            raise ValueError("every image must be a contiguous uint8 tensor [h,w,3]")
        if not (1 <= sh[0] <= MAX_SIDE and 1 <= sh[1] <= MAX_SIDE):
            raise ValueError(f"an image's sides must be 1..{MAX_SIDE}")
        hw.append((sh[0], sh[1]))
    dev = images[0].device
    if any(t.device != dev for t in images):
        raise ValueError("the images must be on one device")
    crops = [(int(y0), int(x0), int(gh), int(gw)) for y0, x0, gh, gw in crops]       # (anything but four numbers: ValueError)
    if len(crops) != B:
        raise ValueError("one (y0, x0, gh, gw) per sample")
    lh, lw = (int(lr_size), int(lr_size)) if isinstance(lr_size, int) else (int(lr_size[0]), int(lr_size[1]))
    if not (1 <= lh <= MAX_SIDE and 1 <= lw <= MAX_SIDE):
        raise ValueError(f"lr_size must be 1..{MAX_SIDE}")
    hf, vf, rt = _flags(hflip, B, "hflip"), _flags(vflip, B, "vflip"), _flags(rot90, B, "rot90")
    for (h, w), (y0, x0, gh, gw), r in zip(hw, crops, rt):
        if gh < 1 or gw < 1:
            raise ValueError("a crop has no pixel")
        if y0 < 0 or x0 < 0 or y0 + gh > h or x0 + gw > w:
            raise ValueError(f"the crop {(y0, x0, gh, gw)} lies outside its image of {h} x {w} pixels")
        if r and (gh != gw or lh != lw):
            raise ValueError("rot90 needs a square crop and a square lr_size: a transposed sample would differ in shape from its neighbours")
        _check_axis(gh, lh, lh / gh, antialiasing)      # the resize's reflection condition
        _check_axis(gw, lw, lw / gw, antialiasing)
    ext = [(gw, gh) if r else (gh, gw) for (_, _, gh, gw), r in zip(crops, rt)]
    if gt_pad is None:
        Gh, Gw = max(e[0] for e in ext), max(e[1] for e in ext)
    else:
        Gh, Gw = int(gt_pad[0]), int(gt_pad[1])
        if any(e[0] > Gh or e[1] > Gw for e in ext) or Gh > MAX_SIDE or Gw > MAX_SIDE:
            raise ValueError(f"gt_pad {(Gh, Gw)} is smaller than a sample (or above {MAX_SIDE})")
    out = {"gt_size": torch.tensor([[gh, gw] for _, _, gh, gw in crops], dtype=torch.int64),
           "scale_modify": torch.tensor([[gh / lh, gw / lw] for _, _, gh, gw in crops], dtype=torch.float32)}
    if sample_coords is not None:
        if not (torch.is_tensor(sample_coords) and not sample_coords.dtype.is_floating_point and sample_coords.dtype != torch.bool
                and sample_coords.dim() == 3 and sample_coords.shape[0] == B and sample_coords.shape[1] >= 1
                and sample_coords.shape[2] == 2 and sample_coords.device == dev):
            raise ValueError("sample_coords must be an integer tensor [B,S,2] on the images' device")
        out["sample_coords"] = sample_coords
    else:
        out["pad_h"], out["pad_w"] = Gh - out["gt_size"][:, 0], Gw - out["gt_size"][:, 1]      # (a transposed sample is square)
    if dev.type == "cuda":
        from . import _cabi
        aug = [(_cabi.BATCH_HFLIP if h else 0) | (_cabi.BATCH_VFLIP if v else 0) | (_cabi.BATCH_TRANSPOSE if r else 0)
               for h, v, r in zip(hf, vf, rt)]
        ptrs = [t.data_ptr() for t in images]      # (checked above)
        with _cabi._on(dev):
            lq = torch.empty(B, 3, lh, lw, dtype=torch.float32, device=dev)
            if sample_coords is None:
                gt = torch.empty(B, 3, Gh, Gw, dtype=torch.float32, device=dev)
                _cabi._batch_make(dev, ptrs, hw, crops, aug, gt, lq, bgr, antialiasing)
            else:
                _cabi._batch_make(dev, ptrs, hw, crops, aug, None, lq, bgr, antialiasing)       # (the LR images only)
                gt = torch.empty(B, 3, sample_coords.shape[1], dtype=torch.float32, device=dev)
                _cabi._batch_pick(dev, ptrs, hw, crops, aug, sample_coords.to(torch.int32).contiguous(), gt, bgr)
        out["gt"], out["lq"] = gt, lq
        return out
    gts, lqs = [], []
    for b, (t, (y0, x0, gh, gw)) in enumerate(zip(images, crops)):
        chw = (t[y0:y0 + gh, x0:x0 + gw].float() / 255).permute(2, 0, 1)
        chw = chw.flip(0) if bgr else chw
        lqs.append(_augment(resize_torch(chw, (lh, lw), (lh / gh, lw / gw), antialiasing), hf[b], vf[b], rt[b]))
        g = _augment(chw, hf[b], vf[b], rt[b])
        if sample_coords is None:
            slot = torch.zeros(3, Gh, Gw, dtype=torch.float32)
            slot[:, :g.shape[1], :g.shape[2]] = g
        else:
            p = sample_coords[b].long()
            r, c = p[:, 0], p[:, 1]
            r, c = torch.where(r < 0, r + g.shape[1], r), torch.where(c < 0, c + g.shape[2], c)
            ok = (r >= 0) & (r < g.shape[1]) & (c >= 0) & (c < g.shape[2])
            slot = g[:, r.clamp(0, g.shape[1] - 1), c.clamp(0, g.shape[2] - 1)] * ok.to(torch.float32)
        gts.append(slot)
    out["gt"], out["lq"] = torch.stack(gts), torch.stack(lqs)
    return out


def draw_batch(image_sizes, lr_size, scale_list, rng, round_mode="ceil", use_hflip=True, use_rot=True, cap_scale_to_image=False):
    """The dataset's random draws for a batch, on the host, from `rng` (a `random.Random`) in the dataset's own order and by
    its own rules, sample after sample:

    the scale, `rng.uniform(*scale_list)` for a two-element list (with `cap_scale_to_image`, the `_sa1b` rule, its upper end is
    `min(h / lr, w / lr, scale_list[1])`), `rng.choice(scale_list)` otherwise; `gt_size` = `ceil(scale * lr)` -- on the float32
    product, as the reference's `scale * torch.tensor(lr)` is one -- or Python's `round(scale * lr)` per `round_mode`; the two
    inclusive offsets `rng.randint(0, h - gh)`, `rng.randint(0, w - gw)`; then `rng.random() < 0.5` once for `hflip` only if
    `use_hflip`, and twice for `vflip` and `rot90` only if `use_rot` (the reference's `and` short-circuits the draws).

    `image_sizes`: one `(h, w)` per sample; `lr_size`: an int or `(lh, lw)` (`use_rot` needs it square).  Returns
    `(args, scales)`: `args` = {'crops', 'hflip', 'vflip', 'rot90'}, the keyword arguments of `make_batch`, and the drawn scales.
    ValueError where an image is smaller than its crop (the reference's `randint` raises there)."""
    lh, lw = (int(lr_size), int(lr_size)) if isinstance(lr_size, int) else (int(lr_size[0]), int(lr_size[1]))
    if round_mode not in ("ceil", "round"):
        raise ValueError("round_mode must be 'ceil' or 'round'")
    if use_rot and lh != lw:
        raise ValueError("use_rot draws transpositions, which need a square lr_size")
    scale_list = list(scale_list)
    crops, scales, hf, vf, rt = [], [], [], [], []
    for h, w in image_sizes:
        h, w = int(h), int(w)
        if len(scale_list) == 2:
            top = min(min(h / lh, w / lw), scale_list[1]) if cap_scale_to_image else scale_list[1]
            scale = float(rng.uniform(scale_list[0], top))
        else:
            scale = rng.choice(scale_list)
        if round_mode == "ceil":
            gh, gw = math.ceil(scale * torch.tensor(lh)), math.ceil(scale * torch.tensor(lw))
        else:
            gh, gw = round(scale * lh), round(scale * lw)
        if gh < 1 or gw < 1 or gh > h or gw > w:
            raise ValueError(f"an image of {h} x {w} pixels cannot hold a crop of {gh} x {gw}")
        y0 = rng.randint(0, h - gh)
        x0 = rng.randint(0, w - gw)
        crops.append((y0, x0, gh, gw))
        scales.append(scale)
        hf.append(bool(use_hflip and rng.random() < 0.5))
        vf.append(bool(use_rot and rng.random() < 0.5))
        rt.append(bool(use_rot and rng.random() < 0.5))
    return {"crops": crops, "hflip": hf, "vflip": vf, "rot90": rt}, scales
