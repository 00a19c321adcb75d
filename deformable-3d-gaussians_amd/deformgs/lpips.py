"""lpips(): LPIPS-VGG (lpips.LPIPS(net='vgg'), version 0.1) of N frame pairs through dgs_lpips (csrc/lpips.hip).

The weights are the user's: torchvision's VGG16 state dict and the LPIPS linear-layer file. Nothing here ships
or fetches them. load_weights() reads the two files, weights_from_tensors() takes the same tensors from memory;
both repack them once into the layout dgs_lpips reads (include/dgs.h).

Images are taken as given: the reference's metrics.py passes [0, 1] images without the 2v - 1 step, so
normalize=False is the default. One call is a fixed number of launches per chunk of frames and waits for
nothing: the results are device tensors.

Scratch: two activation buffers of 2 * 64 * H * W floats per frame pair, about 1 KiB per pixel of a pair (625
MiB at 800 x 800). Frames are walked in chunks that fit `scratch_bytes` (DEFAULT_SCRATCH_BYTES = 2 GiB: three
pairs at 800 x 800, which already fills the device; a budget below one pair's need still takes one pair at a
time), through one allocation, with no read-back between chunks. Chunking changes no bit of the result.
"""
import torch

CONV_KEYS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)  # torchvision VGG16 features.N
CONV_CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512)
CONV_COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
TAP_CHANNELS = (64, 128, 256, 512, 512)
MIN_SIDE = 16  # four 2x2 pools
DEFAULT_SCRATCH_BYTES = 2 << 30
NORMALIZE = 1  # DGS_LPIPS_NORMALIZE (include/dgs.h)
_KC = 16  # input channels per K chunk of the convolution kernel


class LpipsWeights:
    """The packed device buffer dgs_lpips reads."""

    def __init__(self, packed):
        self.packed = packed

    @property
    def device(self):
        return self.packed.device


def _pack_conv(w):
    """(Cout, Cin, 3, 3) -> [Cin_p / 16][Cout][ky * 3 + kx][16], Cin_p = Cin rounded up to 16 with zeros."""
    cout, cin = w.shape[:2]
    cin_p = -(-cin // _KC) * _KC
    p = torch.zeros((cout, cin_p, 3, 3), dtype=torch.float32)
    p[:, :cin] = w
    return p.view(cout, cin_p // _KC, _KC, 9).permute(1, 0, 3, 2).contiguous().flatten()


def weights_from_tensors(conv_weights, conv_biases, lins, device):
    """conv_weights: 13 tensors (Cout, Cin, 3, 3) in VGG16 order, conv_biases: 13 of (Cout,), lins: 5 of C (any
    shape with C elements, e.g. (1, C, 1, 1)) -> LpipsWeights on `device`. ValueError names a wrong shape."""
    if len(conv_weights) != 13 or len(conv_biases) != 13 or len(lins) != 5:
        raise ValueError("lpips: expected 13 convolution weights, 13 biases and 5 linear layers")
    parts = []
    for i, (w, b) in enumerate(zip(conv_weights, conv_biases)):
        want = (CONV_COUT[i], CONV_CIN[i], 3, 3)
        if tuple(w.shape) != want:
            raise ValueError(f"lpips: convolution {i} weight has shape {tuple(w.shape)}, expected {want}")
        if tuple(b.shape) != (CONV_COUT[i],):
            raise ValueError(f"lpips: convolution {i} bias has shape {tuple(b.shape)}, expected {(CONV_COUT[i],)}")
        parts += [_pack_conv(w.detach().cpu().float()), b.detach().cpu().float()]
    for k, lin in enumerate(lins):
        if lin.numel() != TAP_CHANNELS[k]:
            raise ValueError(f"lpips: linear layer {k} has shape {tuple(lin.shape)}, expected {TAP_CHANNELS[k]} weights")
        parts.append(lin.detach().cpu().float().flatten())
    packed = torch.cat(parts)
    from . import _lib
    assert packed.numel() == _lib.load().dgs_lpips_weight_floats()
    return LpipsWeights(packed.to(device))


def _pick(sd, names, path):
    for n in names:
        if n in sd:
            return n, sd[n]
    raise ValueError(f"lpips: {path}: missing key {names[0]!r} (also tried {', '.join(map(repr, names[1:]))})")


def load_weights(vgg_path, lin_path, device):
    """vgg_path: torchvision's VGG16 state dict (keys features.N.weight / features.N.bias, or the same without
    the features. prefix; other keys are ignored). lin_path: the LPIPS linear-layer file (keys
    linK.model.1.weight, or K.1.weight, of shape (1, C, 1, 1)). A missing key or a wrong shape raises a
    ValueError that names it."""
    vgg = torch.load(vgg_path, map_location="cpu", weights_only=True)
    lin = torch.load(lin_path, map_location="cpu", weights_only=True)
    ws, bs, ls = [], [], []
    for i, n in enumerate(CONV_KEYS):
        for kind, dst, want in (("weight", ws, (CONV_COUT[i], CONV_CIN[i], 3, 3)), ("bias", bs, (CONV_COUT[i],))):
            key, t = _pick(vgg, (f"features.{n}.{kind}", f"{n}.{kind}"), vgg_path)
            if tuple(t.shape) != want:
                raise ValueError(f"lpips: {vgg_path}: {key!r} has shape {tuple(t.shape)}, expected {want}")
            dst.append(t)
    for k, c in enumerate(TAP_CHANNELS):
        key, t = _pick(lin, (f"lin{k}.model.1.weight", f"{k}.1.weight"), lin_path)
        if tuple(t.shape) != (1, c, 1, 1):
            raise ValueError(f"lpips: {lin_path}: {key!r} has shape {tuple(t.shape)}, expected {(1, c, 1, 1)}")
        ls.append(t)
    return weights_from_tensors(ws, bs, ls, device)


def _batch(x, what):
    if isinstance(x, (list, tuple)):
        if not x:
            raise ValueError(f"lpips: empty list of {what}")
        if any(not torch.is_tensor(t) for t in x):
            raise ValueError(f"lpips: {what} must be tensors")
        if any(t.shape != x[0].shape for t in x):
            raise ValueError(f"lpips: {what} of different sizes in one call: {sorted({tuple(t.shape) for t in x})}")
        x = torch.stack(list(x)) if x[0].dim() == 3 else torch.cat(list(x))
    if not torch.is_tensor(x):
        raise ValueError(f"lpips: {what} must be a tensor or a list of tensors")
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dim() != 4:
        raise ValueError(f"lpips: {what} must be (F, 3, H, W) or (3, H, W), got {tuple(x.shape)}")
    if x.shape[1] != 3:
        raise ValueError(f"lpips: {what} must have 3 channels, got {tuple(x.shape)}")
    if min(x.shape[2], x.shape[3]) < MIN_SIDE:
        raise ValueError(f"lpips: needs min(H, W) >= {MIN_SIDE} (four 2x2 pools); got {x.shape[2]} x {x.shape[3]}")
    return x


def _prepare(x, weights):
    from . import _lib
    _lib.require_cuda(x)
    if not isinstance(weights, LpipsWeights):
        raise ValueError("lpips: weights must come from load_weights() or weights_from_tensors()")
    if x.device != weights.device:
        raise ValueError(f"lpips: images on {x.device}, weights on {weights.device}")
    return x.float().contiguous()


def lpips(renders, gts, weights, normalize=False, return_layers=False, scratch_bytes=None):
    """renders, gts: (F, 3, H, W) or (3, H, W) device float tensors, or lists of such of one size.
    -> (F,) device tensor of LPIPS-VGG; with return_layers also the (F, 5) layer terms it is the sum of.
    normalize: map both through 2v - 1 first. scratch_bytes: the budget the frames are chunked to (module
    docstring). Raises ValueError on CPU tensors (there is no fallback), C != 3, mismatched shapes and
    min(H, W) < 16."""
    a, b = _batch(renders, "renders"), _batch(gts, "gts")
    if a.shape != b.shape:
        raise ValueError(f"lpips: renders {tuple(a.shape)} and gts {tuple(b.shape)} differ in shape")
    from . import _lib
    a, b = _prepare(a, weights), _prepare(b, weights)
    lib = _lib.load()
    F, _, H, W = a.shape
    one = lib.dgs_lpips_scratch_bytes(1, H, W)
    budget = DEFAULT_SCRATCH_BYTES if scratch_bytes is None else int(scratch_bytes)
    per = max(1, min(F, budget // one))
    out = torch.empty((F, 6), dtype=torch.float32, device=a.device)
    scratch = torch.empty(per * one, dtype=torch.uint8, device=a.device)
    flags = NORMALIZE if normalize else 0
    with torch.cuda.device(a.device):
        for i in range(0, F, per):
            n = min(per, F - i)
            _lib.check(lib.dgs_lpips(n, H, W, _lib.ptr(a[i:]), _lib.ptr(b[i:]), _lib.ptr(weights.packed), flags,
                                     _lib.ptr(out[i:]), None, _lib.ptr(scratch), _lib.stream_ptr(a.device)), "lpips")
    return (out[:, 5], out[:, :5]) if return_layers else out[:, 5]


def vgg_taps(x, weights, normalize=False):
    """The five taps (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3) of x: (F, 3, H, W) or (3, H, W) device
    tensor -> five (F, C, Hk, Wk) tensors. For tests: the whole batch runs as one chunk."""
    from . import _lib
    x = _prepare(_batch(x, "images"), weights)
    lib = _lib.load()
    F, _, H, W = x.shape
    shapes, h, w = [], H, W
    for c in TAP_CHANNELS:
        shapes.append((F, h, w, c))
        h, w = h // 2, w // 2
    sizes = [s[0] * s[1] * s[2] * s[3] for s in shapes]
    taps = torch.empty(sum(sizes), dtype=torch.float32, device=x.device)
    out = torch.empty((F, 6), dtype=torch.float32, device=x.device)
    scratch = torch.empty(lib.dgs_lpips_scratch_bytes(F, H, W), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.dgs_lpips(F, H, W, _lib.ptr(x), _lib.ptr(x), _lib.ptr(weights.packed),
                                 NORMALIZE if normalize else 0, _lib.ptr(out), _lib.ptr(taps), _lib.ptr(scratch),
                                 _lib.stream_ptr(x.device)), "lpips taps")
    return [t.view(s).permute(0, 3, 1, 2) for t, s in zip(taps.split(sizes), shapes)]
