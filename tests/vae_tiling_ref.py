"""numpy restatement of the reference's VAE tiling (`--vae-tiling`), shared by tests/test_vae_tiling_cpu.py and tests/test_gpu_vae_tiling.py.

Written from the rules, in f32 where the rules say f32: tile sizes (VAE::get_tile_sizes), tile count / achieved overlap per axis (sd_tiling_calc_tiles,
non-circular), tile order and the shifted last tile (process_tiles_2d), the blend old + (new * s(y_f)) * s(x_f) with the smootherstep ramp
(sd_tensor_merge_2d).  Arrays are numpy [N, C, H, W] (ggml [W, H, C, N])."""
import math

import numpy as np

F = np.float32


def tile_size(requested, rel, latent, overlap, encode_factor=1.0):
    overlap = F(max(min(F(overlap), F(0.5)), F(0.0)))
    size = 32
    rel = F(rel)
    if rel > 0:
        if rel > 1.0:
            rel = F(1) / F(F(rel - F(rel * overlap)) + overlap)
        size = int(math.floor(float(F(F(latent) * rel)) + 0.5))   # std::round of a positive float
    elif requested >= 4:
        size = requested
    size = int(F(F(size) * F(encode_factor)))
    return max(min(size, latent), 4)


def axis(small, requested, target):
    """-> (tile, overlap, [(start, skip), ...]) in latent cells"""
    target = F(max(min(F(target), F(0.5)), F(0.0)))
    want = int(F(requested) * target)
    stride0 = requested - want
    count = (small - want) // stride0
    over = ((count + 1) * stride0 + want) % small
    if over != stride0 and over <= count * (requested // 2 - want):
        count += 1
    if count <= 2:
        if small <= requested:
            count, factor = 1, F(0)
        else:
            count, factor = 2, F(2 * requested - small) / F(requested)
    else:
        factor = F(requested * count - small) / F(requested * (count - 1))
    overlap = int(F(requested) * factor)
    tile = min(requested, small)
    step = requested - overlap
    pos, x = [], 0
    while x < small:
        if x + tile >= small:
            pos.append((small - tile, x - (small - tile)))
            break
        pos.append((x, 0))
        x += step
    return tile, overlap, pos


def plan(small_w, small_h, tile_size_x=0, tile_size_y=0, target_overlap=0.5, rel_size_x=0.0, rel_size_y=0.0, encode_factor=1.0):
    tx, ox, px = axis(small_w, tile_size(tile_size_x, rel_size_x, small_w, target_overlap, encode_factor), target_overlap)
    ty, oy, py = axis(small_h, tile_size(tile_size_y, rel_size_y, small_h, target_overlap, encode_factor), target_overlap)
    return {"tile_size": (tx, ty), "overlap": (ox, oy), "tiles": [(x, y, dx, dy) for (y, dy) in py for (x, dx) in px]}


def ramp(t):
    t = np.asarray(t, F)
    return t * t * t * (t * (F(6) * t - F(15)) + F(10))


def weights(tile, start, skip, overlap, full):
    """s(min(rise, fall, 1)) for the cells skip .. tile-1 of one tile along one axis (output cells)"""
    i = np.arange(skip, tile)
    one = np.ones(len(i), F)
    rise = (i - skip).astype(F) / F(overlap) if (overlap > 0 and start > 0) else one
    fall = (tile - i).astype(F) / F(overlap) if (overlap > 0 and start < full - tile) else one
    return ramp(np.minimum(np.minimum(rise, fall), F(1)))


def merge(canvas, tile, x, y, ovx, ovy, dx, dy):
    """sd_tensor_merge_2d on every plane at once: canvas [N, C, H, W] (modified in place), tile [N, C, th, tw]; all geometry in output cells"""
    th, tw = tile.shape[-2:]
    H, W = canvas.shape[-2:]
    new = tile[..., dy:, dx:]
    dst = canvas[..., y + dy:y + th, x + dx:x + tw]
    if ovx > 0 or ovy > 0:
        sx = weights(tw, x, dx, ovx, W)
        sy = weights(th, y, dy, ovy, H)
        dst[...] = dst + (new * sy[:, None]) * sx[None, :]
    else:
        dst[...] = new


def tiled(x, fn, pl, decode, out_channels):
    """process_tiles_2d: x [N, C, H, W]; fn(crop) -> the model's output for one crop; pl = plan(...) over the latent size"""
    n = x.shape[0]
    tx, ty = pl["tile_size"]
    ovx, ovy = pl["overlap"]
    si, so = (1, 8) if decode else (8, 1)
    sh, sw = (x.shape[2], x.shape[3]) if decode else (x.shape[2] // 8, x.shape[3] // 8)
    canvas = np.zeros((n, out_channels, sh * so, sw * so), F)
    for (px, py, dx, dy) in pl["tiles"]:
        crop = np.ascontiguousarray(x[:, :, py * si:(py + ty) * si, px * si:(px + tx) * si])
        merge(canvas, fn(crop), px * so, py * so, ovx * so, ovy * so, dx * so, dy * so)
    return canvas
