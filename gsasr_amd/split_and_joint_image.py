"""Tiled (memory-bounded) inference driver -- mirror of the reference's `utils/split_and_joint_image.py:98-232`
(`split_and_joint_image`, same name, arguments, defaults and assertions).

The reference cuts the (reflect-padded) LR image into overlapping `split_size` tiles, runs encoder, decoder and
rasterizer tile by tile, and pastes the SR tiles into one canvas, dropping `crop_size` rows/columns on the sides
that overlap an earlier tile.  Here the encoder/decoder callables are still run per tile (they are the caller's),
but the rasterizer runs ALL tiles, as many at a time as fit one batched canvas (64 slots, 32 767 rows), (every tile has the same size,
`gsasr_amd.gaussian_splatting.generate_2D_gaussian_splatting_batch`), and the pasting is one rule instead of the
reference's case tree -- including its one irregularity, kept on purpose: with a fractional scale factor the
reference does not crop the top of a last-column tile (or the left of a last-row tile) that is neither in the
first row/column nor the corner (`:178-185`).

Multi-GPU (not in the reference): with `distribute=True` inside an initialised `torch.distributed` job every rank
runs encoder, decoder and rasterizer for the tiles `rank, rank+world, ...` only and ONE `all_gather` brings the SR
tiles together before pasting -- tiles are independent, so this is the tile shard of SURVEY.md 8e at the level of
the whole pipeline (the caller's models are replicated, as under DDP).
"""
import math

import torch
import torch.nn.functional as F

from .gaussian_splatting import (_batch_step_sizes, _dmax_arg, generate_2D_gaussian_splatting_batch,
                                 generate_2D_gaussian_splatting_step, generate_2D_gaussian_splatting_step_uint8, max_canvas_batch,
                                 quantise_uint8)


def _paste_rule(i, j, nh, nw, crop, fractional):
    """rows / columns of tile (i, j) that are dropped before pasting (reference :160-222)"""
    top, left = (crop if i > 0 else 0), (crop if j > 0 else 0)
    if fractional and i > 0 and j > 0:
        if j == nw - 1 and i != nh - 1:
            top = 0
        elif i == nh - 1 and j != nw - 1:
            left = 0
    return top, left


def tile_places(nh, nw, size_sr, stride_sr, crop, fractional, out_rows=None, out_cols=None):
    """Per tile of the `nh` x `nw` grid, in raster order: the rectangle of the tile that survives in the joined picture when
    the tiles are pasted in raster order under `_paste_rule`, later tiles on top -- `(y0, x0, y1, x1, dst_y, dst_x)`: rows
    `[y0, y1)`, columns `[x0, x1)` of the tile's own `size_sr` grid, whose pixel `(y0, x0)` is picture pixel `(dst_y, dst_x)`
    Empty rectangles have `y1 == y0` or `x1 == x0`.

    Why one rectangle is enough: tile (i, j) pastes rows `[i S + top_ij, i S + size)` and columns `[j S + left_ij, j S + size)`
    (S = `stride_sr`).  What later tiles take away from it is (a) on the right, the columns from `(j + 1) S + left_{i,j+1}` on --
    tile (i, j + 1) never starts lower than (i, j) (`top_{i,j+1} <= top_ij`: the only tile with `top = 0` below the first row
    is in the last column), so it takes those columns over the tile's whole height -- and (b) below, the rows from
    `(i + 1) S + top_{i+1,j}` on: tile (i + 1, j) starts no further right than (i, j) (`left_{i+1,j} <= left_ij`, likewise)
    and is as wide, so it takes those rows over the whole width.  The other tiles of row i + 1 take nothing more: to the left,
    (i + 1, j - 1) starts no higher than (i + 1, j) where the two meet; to the right, what (i + 1, j + 1) covers above
    (i + 1, j) -- the fractional rule's uncropped top in the last column -- lies in the columns (a) has already taken.  Tiles
    further away start later still and end later, so they reach nothing the neighbours have left.  Where `crop` exceeds the
    SR overlap the cut lies beyond the tile's end: the strip between belongs to nobody (and stays zero).
    `out_rows`, `out_cols`: the picture is the top-left corner of the joined extent of that size; the rectangles are clipped."""
    places = []
    for i in range(nh):
        for j in range(nw):
            top, left = _paste_rule(i, j, nh, nw, crop, fractional)
            y1 = size_sr if i == nh - 1 else min(size_sr, stride_sr + _paste_rule(i + 1, j, nh, nw, crop, fractional)[0])
            x1 = size_sr if j == nw - 1 else min(size_sr, stride_sr + _paste_rule(i, j + 1, nh, nw, crop, fractional)[1])
            dst_y, dst_x = i * stride_sr + top, j * stride_sr + left
            if out_rows is not None:
                y1 = min(y1, top + out_rows - dst_y)
            if out_cols is not None:
                x1 = min(x1, left + out_cols - dst_x)
            y1, x1 = max(y1, top), max(x1, left)
            places.append((top, left, y1, x1, dst_y, dst_x))
    return places


def _tile_groups(n_tiles, tile_batch, per_canvas):
    """the tiles 0 .. n_tiles - 1 in raster order, in groups of at most min(tile_batch, per_canvas); a last group of ONE tile
    takes a tile from the group before it (a canvas has at least two samples) where that group has one to spare -- groups of
    two have none: an odd number of tiles at tile_batch=2 ends in a single tile, which is rendered as a single image"""
    g = max(1, min(int(tile_batch), int(per_canvas)))
    groups = [list(range(a, min(a + g, n_tiles))) for a in range(0, n_tiles, g)]
    if len(groups) > 1 and len(groups[-1]) == 1 and len(groups[-2]) > 2:
        groups[-1].insert(0, groups[-2].pop())
    return groups


def _joined_tiles(lq_pad, nh, nw, stride, split_size, size_sr, stride_sr, scale_factor, model_g, model_fea2gs, scale_modify,
                  crop_size, default_step_size, mode, cuda_rendering, if_dmax, dmax_mode, dmax, out_uint8, bgr, tile_batch, out_size):
    """`split_and_joint_image(tile_batch=k)`: the picture is allocated once; a group of tiles is encoded, decoded, rendered (on
    the GPU as one batched canvas of the group) and the rectangle each tile owns (`tile_places`) assigned to its place; the
    group's Gaussians, plan workspace and canvas are dropped before the next group: besides the picture, memory is per group
    (a group of all tiles saves nothing)."""
    dev = lq_pad.device
    full = ((nh - 1) * stride_sr + size_sr, (nw - 1) * stride_sr + size_sr)
    rows, cols = full if out_size is None else (int(out_size[0]), int(out_size[1]))
    if not (1 <= rows <= full[0] and 1 <= cols <= full[1]):
        raise ValueError(f"out_size-{(rows, cols)} must lie inside the joined picture-{full}")
    fractional = scale_factor != int(scale_factor)
    places = tile_places(nh, nw, size_sr, stride_sr, crop_size, fractional, rows, cols)
    # zeros: the pixels that no tile owns (crop_size above the SR overlap) are zero, as in the pasted canvas
    sr = torch.zeros((rows, cols, 3), dtype=torch.uint8, device=dev) if out_uint8 else torch.zeros((3, rows, cols), dtype=torch.float32, device=dev)
    on_gpu = bool(cuda_rendering and lq_pad.is_cuda)
    dm = None
    if on_gpu:
        from . import _cabi
        dm = _dmax_arg(dmax, dmax_mode, if_dmax, (size_sr, size_sr))
    for group in _tile_groups(nh * nw, tile_batch, max_canvas_batch(size_sr)):
        params = []
        for k in group:
            i, j = divmod(k, nw)
            tile = lq_pad[:, :, i * stride: i * stride + split_size, j * stride: j * stride + split_size]
            feat = model_g(tile)
            scale_vector = scale_modify[0].unsqueeze(0).to(feat.device)
            params.append(model_fea2gs(feat, scale_vector)[0, :])
        if on_gpu and len(group) > 1:
            # one batched canvas of the group's tiles (the rasterizer's own batched step); each tile's owned rectangle is then
            # assigned to its place -- the canvas lives until the next group's replaces it
            gp = torch.stack(params).detach().float().contiguous()
            steps = _batch_step_sizes([scale_factor] * len(group), [scale_modify] * len(group), default_step_size, mode, gp.device)
            sizes = [(size_sr, size_sr)] * len(group)
            if out_uint8:
                canvas = _cabi.batch_forward_u8(gp, steps, sizes, dm, bgr=bgr)[0]                       # [G, size, size, 3]
            else:
                canvas = _cabi.batch_forward(gp, steps, sizes, dm, _cabi.FLAG_FORWARD_ONLY)[0]          # [G, 3, slot, size]
            for b, k in enumerate(group):
                y0, x0, y1, x1, dy, dx = places[k]
                if y1 <= y0 or x1 <= x0:
                    continue
                if out_uint8:
                    sr[dy: dy + y1 - y0, dx: dx + x1 - x0] = canvas[b, y0: y1, x0: x1]
                else:
                    sr[:, dy: dy + y1 - y0, dx: dx + x1 - x0] = canvas[b, :, y0: y1, x0: x1]
            del gp, canvas
        else:   # CPU tensors, cuda_rendering=False, or a group of ONE tile (tile_batch=2 on an odd number of tiles leaves one
            # over; a canvas that holds a single tile): tile by tile through the single-image calls
            for k, p in zip(group, params):
                y0, x0, y1, x1, dy, dx = places[k]
                if y1 <= y0 or x1 <= x0:
                    continue
                if out_uint8 and on_gpu:
                    img = generate_2D_gaussian_splatting_step_uint8(torch.tensor([size_sr, size_sr]), p, scale_factor, scale_modify,
                                                                    default_step_size=default_step_size, mode=mode, if_dmax=if_dmax,
                                                                    dmax_mode=dmax_mode, dmax=dmax, bgr=bgr)
                    sr[dy: dy + y1 - y0, dx: dx + x1 - x0] = img[y0: y1, x0: x1]
                    continue
                img = generate_2D_gaussian_splatting_step(sr_size=torch.tensor([size_sr, size_sr]), gs_parameters=p, scale=scale_factor,
                                                          sample_coords=None, scale_modify=scale_modify,
                                                          default_step_size=default_step_size, mode=mode, cuda_rendering=cuda_rendering,
                                                          if_dmax=if_dmax, dmax_mode=dmax_mode, dmax=dmax)
                if out_uint8:
                    sr[dy: dy + y1 - y0, dx: dx + x1 - x0] = quantise_uint8(img, None, bgr)[y0: y1, x0: x1]
                else:
                    sr[:, dy: dy + y1 - y0, dx: dx + x1 - x0] = img[:, y0: y1, x0: x1]
        del params
    return sr if out_uint8 else sr.unsqueeze(0)


def _tiles_uint8(params, size_sr, scale_factor, scale_modify, default_step_size, mode, cuda_rendering, if_dmax, dmax_mode,
                 dmax, bgr):
    """the SR tiles of `params` as uint8 `[size_sr, size_sr, 3]` each: on the GPU through the batched 8-bit canvas (the
    forward kernels store the bytes; a lone tile through the single-image call), otherwise the float tile quantised"""
    tiles = []
    if cuda_rendering and params and params[0].is_cuda:
        from . import _cabi
        per_canvas = max_canvas_batch(size_sr)
        dm = _dmax_arg(dmax, dmax_mode, if_dmax, (size_sr, size_sr))
        for a in range(0, len(params), per_canvas):
            chunk = params[a: a + per_canvas]
            if len(chunk) == 1:
                break
            gp = torch.stack(chunk).detach().float().contiguous()
            steps = _batch_step_sizes([scale_factor] * len(chunk), [scale_modify] * len(chunk), default_step_size, mode, gp.device)
            out, _ = _cabi.batch_forward_u8(gp, steps, [(size_sr, size_sr)] * len(chunk), dm, bgr=bgr)
            tiles.extend(out[k] for k in range(len(chunk)))
        for k in range(len(tiles), len(params)):
            tiles.append(generate_2D_gaussian_splatting_step_uint8(torch.tensor([size_sr, size_sr]), params[k], scale_factor,
                                                                   scale_modify, default_step_size=default_step_size, mode=mode,
                                                                   if_dmax=if_dmax, dmax_mode=dmax_mode, dmax=dmax, bgr=bgr))
        return tiles
    for p in params:
        img = generate_2D_gaussian_splatting_step(sr_size=torch.tensor([size_sr, size_sr]), gs_parameters=p, scale=scale_factor,
                                                  sample_coords=None, scale_modify=scale_modify,
                                                  default_step_size=default_step_size, mode=mode, cuda_rendering=cuda_rendering,
                                                  if_dmax=if_dmax, dmax_mode=dmax_mode, dmax=dmax)
        tiles.append(quantise_uint8(img, None, bgr))
    return tiles


def split_and_joint_image(lq, scale_factor, split_size, overlap_size, model_g, model_fea2gs, scale_modify,
                          crop_size=2, default_step_size=1.2, mode='scale_modify', cuda_rendering=True,
                          if_dmax=False, dmax_mode='fix', dmax=25, distribute=False, group=None, out_uint8=False, bgr=False,
                          tile_batch=None, out_size=None):
    """`tile_batch=k` (k >= 2; not in the reference): bounded memory -- the picture is allocated once and the tiles are encoded,
    decoded, rendered and assigned to it in groups of at most k (`_joined_tiles`), for the float result and for `out_uint8`;
    one image, one rank.  `out_size=(rows, cols)` (with `tile_batch`): the reference callers' `[:gt_h, :gt_w]` of the result,
    never rendered beyond.  `tile_batch=None`: everything below, as it always was.
    `out_uint8=True` (not in the reference): the result as the 8-bit picture uint8 `[H, W, 3]` (`bgr`: b, g, r order) that
    the reference's callers make of the float canvas -- clamp(0, 1), HWC, `(x * 255).round()` -- with the tiles rendered,
    gathered across ranks and pasted as uint8 (a quarter of the bytes).  One image only."""
    h_lq, w_lq = lq.shape[-2:]
    assert overlap_size > 0 and overlap_size < split_size // 2, f"overlap size is wrong"
    stride = split_size - overlap_size
    nh, nw = math.ceil((h_lq - overlap_size) / stride), math.ceil((w_lq - overlap_size) / stride)
    pad_h, pad_w = nh * stride + overlap_size - h_lq, nw * stride + overlap_size - w_lq
    assert pad_h < h_lq, f'pad_h_lq-{pad_h} should be smaller than h_lq-{h_lq}, please decrease the split_size-{split_size}'
    assert pad_w < w_lq, f'pad_w_lq-{pad_w} should be smaller than w_lq-{w_lq}, please decrease the split_size-{split_size}'
    lq_pad = F.pad(input=lq, pad=(0, pad_w, 0, pad_h), mode='reflect')

    size_sr = math.ceil(split_size * scale_factor)
    n_tiles = nh * nw
    if tile_batch is None:
        if out_size is not None:
            raise ValueError("out_size needs tile_batch")
    else:
        if int(tile_batch) < 2:
            raise ValueError(f"tile_batch-{tile_batch} must be at least 2")
        if lq.shape[0] != 1:
            raise ValueError(f"tile_batch joins one image, lq has batch-{lq.shape[0]}")
        if distribute and torch.distributed.is_available() and torch.distributed.is_initialized() \
                and torch.distributed.get_world_size(group) > 1:
            raise ValueError("tile_batch does not combine with distribute=True on more than one rank")
        overlap_sr = math.ceil(overlap_size * scale_factor)
        return _joined_tiles(lq_pad, nh, nw, stride, split_size, size_sr, size_sr - overlap_sr, scale_factor, model_g, model_fea2gs,
                             scale_modify, crop_size, default_step_size, mode, cuda_rendering, if_dmax, dmax_mode, dmax, out_uint8,
                             bgr, tile_batch, out_size)
    rank, world = 0, 1
    if distribute and torch.distributed.is_available() and torch.distributed.is_initialized():
        rank, world = torch.distributed.get_rank(group), torch.distributed.get_world_size(group)
    mine = list(range(rank, n_tiles, world))      # this rank's tiles (raster index)

    # encoder + decoder per tile (the caller's models)
    params = []
    for k in mine:
        i, j = divmod(k, nw)
        tile = lq_pad[:, :, i * stride: i * stride + split_size, j * stride: j * stride + split_size]
        feat = model_g(tile)
        scale_vector = scale_modify[0].unsqueeze(0).to(feat.device)
        params.append(model_fea2gs(feat, scale_vector)[0, :])

    if out_uint8:
        assert lq.shape[0] == 1, f'out_uint8 pastes one image, lq has batch-{lq.shape[0]}'
        tiles = _tiles_uint8(params, size_sr, scale_factor, scale_modify, default_step_size, mode, cuda_rendering, if_dmax,
                             dmax_mode, dmax, bgr)
        if world > 1:   # the same all_gather, on uint8 stacks
            per = (n_tiles + world - 1) // world
            stack = torch.zeros(per, size_sr, size_sr, 3, dtype=torch.uint8, device=lq.device)
            if tiles:
                stack[: len(tiles)] = torch.stack(tiles)
            everyone = torch.empty(world * per, size_sr, size_sr, 3, dtype=torch.uint8, device=lq.device)
            torch.distributed.all_gather_into_tensor(everyone, stack, group=group)
            tiles = [everyone[(k % world) * per + k // world] for k in range(n_tiles)]
        assert tiles[0].shape[0] == size_sr and tiles[0].shape[1] == size_sr, \
            f'tile_sr_h-{tiles[0].shape[0]}, tile_sr_w-{tiles[0].shape[1]}, split_size_sr-{size_sr} is not the same'
        overlap_sr = math.ceil(overlap_size * scale_factor)
        stride_sr = size_sr - overlap_sr
        sr = torch.zeros((nh - 1) * stride_sr + size_sr, (nw - 1) * stride_sr + size_sr, 3, dtype=torch.uint8, device=lq.device)
        fractional = scale_factor != int(scale_factor)
        for i in range(nh):
            for j in range(nw):
                top, left = _paste_rule(i, j, nh, nw, crop_size, fractional)
                y0, x0 = i * stride_sr, j * stride_sr
                sr[y0 + top: y0 + size_sr, x0 + left: x0 + size_sr] = tiles[i * nw + j][top:, left:]
        return sr

    # rasterizer: all tiles have the same size and scale -> batched canvases of up to 64 tiles
    tiles = []
    if cuda_rendering and params and params[0].is_cuda and len(params) > 1:
        # tiles per canvas: 64 slots, 32 767 canvas rows (17 tiles of the reference's default 480-px tile at x4)
        per_canvas = max_canvas_batch(size_sr)
        for a in range(0, len(params), per_canvas):
            chunk = params[a: a + per_canvas]
            if len(chunk) == 1:
                break
            out = generate_2D_gaussian_splatting_batch([(size_sr, size_sr)] * len(chunk), torch.stack(chunk),
                                                       [scale_factor] * len(chunk), [scale_modify] * len(chunk),
                                                       default_step_size=default_step_size, mode=mode, if_dmax=if_dmax,
                                                       dmax_mode=dmax_mode, dmax=dmax)
            tiles.extend(out[k] for k in range(len(chunk)))
    for k in range(len(tiles), len(params)):
        tiles.append(generate_2D_gaussian_splatting_step(sr_size=torch.tensor([size_sr, size_sr]), gs_parameters=params[k],
                                                         scale=scale_factor, sample_coords=None, scale_modify=scale_modify,
                                                         default_step_size=default_step_size, mode=mode,
                                                         cuda_rendering=cuda_rendering, if_dmax=if_dmax,
                                                         dmax_mode=dmax_mode, dmax=dmax))
    if world > 1:   # one all_gather of equally sized stacks (ranks with one tile less pad with zeros)
        per = (n_tiles + world - 1) // world
        stack = lq.new_zeros(per, lq.shape[1], size_sr, size_sr)
        if tiles:
            stack[: len(tiles)] = torch.stack(tiles)
        everyone = lq.new_empty(world * per, lq.shape[1], size_sr, size_sr)
        torch.distributed.all_gather_into_tensor(everyone, stack, group=group)
        tiles = [everyone[(k % world) * per + k // world] for k in range(n_tiles)]
    assert tiles[0].shape[1] == size_sr and tiles[0].shape[2] == size_sr, \
        f'tile_sr_h-{tiles[0].shape[1]}, tile_sr_w-{tiles[0].shape[2]}, split_size_sr-{size_sr} is not the same'

    # paste in raster order (later tiles overwrite earlier ones where they overlap, as in the reference)
    overlap_sr = math.ceil(overlap_size * scale_factor)
    stride_sr = size_sr - overlap_sr
    sr = torch.zeros(lq.shape[0], lq.shape[1], (nh - 1) * stride_sr + size_sr, (nw - 1) * stride_sr + size_sr,
                     device=lq.device)
    fractional = scale_factor != int(scale_factor)
    for i in range(nh):
        for j in range(nw):
            top, left = _paste_rule(i, j, nh, nw, crop_size, fractional)
            y0, x0 = i * stride_sr, j * stride_sr
            sr[:, :, y0 + top: y0 + size_sr, x0 + left: x0 + size_sr] = tiles[i * nw + j].unsqueeze(0)[:, :, top:, left:]
    return sr
