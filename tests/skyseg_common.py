"""Helper of the sky-segmentation tests (not a conftest): a writer for the ncnn .param / .bin format, builders of the
U^2-Net-small topology and of small operator nets with seeded weights, and the checker -- the graph read back from the very
same files and evaluated by torch on the CPU in float64 (and, as the control, in float32).  Nothing here needs a GPU or any
file from outside the repository."""
import os

import numpy as np

FP16_TAG = 0x01306B47


# ------------------------------------------------------------------------------------------------------------------
# graph builder: layers are recorded without Split; emit() inserts the Splits the way ncnn's converter does (right after
# the producer, the k-th reader of n in file order takes output n - 1 - k)
# ------------------------------------------------------------------------------------------------------------------
class Graph:
    def __init__(self, in_c, h, w, input_name="in0", input_params=True):
        self.layers = []  # (type, name, [in blobs], out blob, params dict)
        self.shape = {}
        self._n = 0
        self.input_name = input_name
        self.shape[input_name] = (in_c, h, w)
        prm = {0: w, 1: h, 2: in_c} if input_params else {}
        self.layers.append(("Input", input_name, [], input_name, prm))

    def _new(self, kind, shape):
        self._n += 1
        name = f"{kind}{self._n}"
        self.shape[name] = shape
        return name

    def conv(self, x, cout, k=3, dil=1, act=1, bias=True, name=None):
        c, h, w = self.shape[x]
        out = self._new("c", (cout, h, w))
        if name:  # a blob name of the caller's choice (the reference extracts the blob "1959")
            self.shape[name] = self.shape.pop(out)
            out = name
        prm = {0: cout, 1: k}
        if dil != 1:
            prm[2] = dil
        pad = dil * (k - 1) // 2
        if pad:
            prm[4] = pad
        if bias:
            prm[5] = 1
        prm[6] = cout * c * k * k
        if act:
            prm[9] = act
        self.layers.append(("Convolution", "Conv_" + out, [x], out, prm))
        return out

    def pool(self, x):
        c, h, w = self.shape[x]
        out = self._new("p", (c, (h + 1) // 2, (w + 1) // 2))
        self.layers.append(("Pooling", "MaxPool_" + out, [x], out, {1: 2, 2: 2}))
        return out

    def interp(self, x, oh, ow):
        c, h, w = self.shape[x]
        out = self._new("r", (c, oh, ow))
        self.layers.append(("Interp", "Resize_" + out, [x], out, {0: 2, 3: oh, 4: ow}))
        return out

    def add(self, a, b):
        out = self._new("a", self.shape[a])
        self.layers.append(("BinaryOp", "Add_" + out, [a, b], out, {}))
        return out

    def concat(self, xs):
        c = sum(self.shape[x][0] for x in xs)
        out = self._new("k", (c,) + self.shape[xs[0]][1:])
        self.layers.append(("Concat", "Concat_" + out, list(xs), out, {}))
        return out

    def sigmoid(self, x):
        out = self._new("s", self.shape[x])
        self.layers.append(("Sigmoid", "Sigmoid_" + out, [x], out, {}))
        return out

    def emit(self):
        """-> list of (type, name, ins, outs, params) with the Split layers in place"""
        readers = {}
        for li, (_, _, ins, _, _) in enumerate(self.layers):
            for pos, b in enumerate(ins):
                readers.setdefault(b, []).append((li, pos))
        rename = {}  # (layer index, input position) -> blob name
        out = []
        nsplit = 0
        for li, (t, name, ins, ob, prm) in enumerate(self.layers):
            ins2 = [rename.get((li, pos), b) for pos, b in enumerate(ins)]
            out.append((t, name, ins2, [ob], dict(prm)))
            rd = readers.get(ob, [])
            if len(rd) > 1:
                n = len(rd)
                outs = [f"{ob}_splitncnn_{i}" for i in range(n)]
                out.append(("Split", f"splitncnn_{nsplit}", [ob], outs, {}))
                nsplit += 1
                for k, key in enumerate(rd):
                    rename[key] = outs[n - 1 - k]
        return out


def param_text(layers, magic="7767517"):
    blobs = set()
    for _, _, ins, outs, _ in layers:
        blobs.update(ins)
        blobs.update(outs)
    lines = [magic, f"{len(layers)} {len(blobs)}"]
    for t, name, ins, outs, prm in layers:
        parts = [f"{t:<24} {name:<24} {len(ins)} {len(outs)}"] + list(ins) + list(outs) + [f"{k}={v}" for k, v in prm.items()]
        lines.append(" ".join(parts))
    return "\n".join(lines) + "\n"


def make_weights(layers, seed, fmt="fp16"):
    """seeded He-scaled weights per Convolution: list of (tag, weights as stored, bias or None).  fmt: 'fp16', 'fp32' or 'mixed'
    (alternating)"""
    rng = np.random.RandomState(seed)
    out = []
    for i, (t, _, _, _, prm) in enumerate(l for l in layers if l[0] == "Convolution"):
        n, cout, k = prm[6], prm[0], prm[1]
        cin = n // (cout * k * k)
        w = (rng.standard_normal(n) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
        b = (rng.standard_normal(cout) * 0.1).astype(np.float32) if prm.get(5, 0) else None
        half = fmt == "fp16" or (fmt == "mixed" and i % 2 == 0)
        out.append((FP16_TAG, w.astype(np.float16), b) if half else (0, w, b))
    return out


def bin_bytes(weights):
    chunks = []
    for tag, w, b in weights:
        chunks.append(np.uint32(tag).tobytes())
        raw = w.tobytes()
        chunks.append(raw + b"\0" * (-len(raw) % 4))
        if b is not None:
            chunks.append(b.astype(np.float32).tobytes())
    return b"".join(chunks)


def write_pair(folder, layers, seed=0, fmt="fp16", stem="net", magic="7767517", weights=None):
    """writes <folder>/<stem>.param and .bin -> (param path, bin path); weights: a list as make_weights returns it, instead of
    seeded ones"""
    os.makedirs(str(folder), exist_ok=True)
    pp, bp = os.path.join(str(folder), stem + ".param"), os.path.join(str(folder), stem + ".bin")
    with open(pp, "w") as f:
        f.write(param_text(layers, magic))
    with open(bp, "wb") as f:
        f.write(bin_bytes(weights if weights is not None else make_weights(layers, seed, fmt)))
    return pp, bp


# ------------------------------------------------------------------------------------------------------------------
# reader + checker
# ------------------------------------------------------------------------------------------------------------------
def read_param(path):
    """-> (declared layer count, declared blob count, [(type, name, ins, outs, {key: str})])"""
    lines = [l.split() for l in open(path).read().strip().split("\n")]
    assert lines[0] == ["7767517"]
    nl, nb = int(lines[1][0]), int(lines[1][1])
    layers = []
    for l in lines[2:]:
        ni, no = int(l[2]), int(l[3])
        prm = dict(x.split("=") for x in l[4 + ni + no:])
        layers.append((l[0], l[1], l[4:4 + ni], l[4 + ni:4 + ni + no], {int(k): v for k, v in prm.items()}))
    return nl, nb, layers


def canonical(layers):
    """the layer list with blobs numbered by first appearance and without layer names: types, parameters, wiring"""
    ids = {}

    def bid(b):
        return ids.setdefault(b, len(ids))

    out = []
    for t, _, ins, outs, prm in layers:
        out.append((t, tuple(bid(b) for b in ins), tuple(bid(b) for b in outs), tuple(sorted((int(k), str(v)) for k, v in prm.items()))))
    return out


def read_weights(layers, bin_path):
    raw = open(bin_path, "rb").read()
    off = 0
    W = {}
    for t, name, _, _, prm in layers:
        if t != "Convolution":
            continue
        n, cout = int(prm[6]), int(prm[0])
        tag = int.from_bytes(raw[off:off + 4], "little")
        off += 4
        if tag == FP16_TAG:
            w = np.frombuffer(raw, np.float16, n, off).astype(np.float32)
            off += (2 * n + 3) // 4 * 4
        else:
            assert tag == 0, hex(tag)
            w = np.frombuffer(raw, np.float32, n, off)
            off += 4 * n
        b = None
        if int(prm.get(5, 0)):
            b = np.frombuffer(raw, np.float32, cout, off)
            off += 4 * cout
        W[name] = (w, b)
    assert off == len(raw), (off, len(raw))
    return W


def evaluate(param_path, bin_path, x, dtype, half_inputs=False):
    """every blob of the graph for input x ([c, h, w] array), computed by torch on the CPU in `dtype` -> {blob name: array [c, h, w]}.
    half_inputs rounds each convolution's input to fp16 first: the arithmetic class the engine must NOT have."""
    import torch
    import torch.nn.functional as F

    _, _, layers = read_param(param_path)
    W = read_weights(layers, bin_path)
    blobs = {}
    for t, name, ins, outs, prm in layers:
        a = [blobs[i] for i in ins]
        if t == "Input":
            r = [torch.from_numpy(np.ascontiguousarray(x))[None].to(dtype)]
        elif t == "Convolution":
            w, b = W[name]
            cout, k, dil, pad, act = int(prm[0]), int(prm[1]), int(prm.get(2, 1)), int(prm.get(4, 0)), int(prm.get(9, 0))
            cin = a[0].shape[1]
            assert int(prm[6]) == cout * cin * k * k
            src = a[0].half().to(dtype) if half_inputs else a[0]
            y = F.conv2d(src, torch.from_numpy(w.copy()).reshape(cout, cin, k, k).to(dtype), torch.from_numpy(b.copy()).to(dtype) if b is not None else None,
                         padding=pad, dilation=dil)
            if act == 1:
                y = F.relu(y)
            elif act == 4:
                y = torch.sigmoid(y)
            else:
                assert act == 0
            r = [y]
        elif t == "Split":
            r = [a[0]] * len(outs)
        elif t == "Pooling":
            assert int(prm.get(0, 0)) == 0 and int(prm[1]) == 2 and int(prm[2]) == 2
            r = [F.max_pool2d(a[0], 2, 2, ceil_mode=True)]
        elif t == "Concat":
            r = [torch.cat(a, 1)]
        elif t == "Interp":
            assert prm[0] == "2"
            r = [F.interpolate(a[0], size=(int(prm[3]), int(prm[4])), mode="bilinear", align_corners=False)]
        elif t == "BinaryOp":
            assert int(prm.get(0, 0)) == 0
            r = [a[0] + a[1]]
        elif t == "Sigmoid":
            r = [torch.sigmoid(a[0])]
        else:
            raise AssertionError(t)
        for o, v in zip(outs, r):
            blobs[o] = v
    return {k: v[0].numpy() for k, v in blobs.items()}


def live_blobs(layers, out):
    """names of the blobs the blob `out` depends on (itself included), from the emitted / read layer list"""
    need = {out}
    for _, _, ins, outs, _ in reversed(layers):
        if need & set(outs):
            need.update(ins)
    return need


def blob_errors(got, ref64):
    """per blob e = max|x - x64| / max|x64| over EVERY element -> {name: e}"""
    out = {}
    for k, r in ref64.items():
        g = np.asarray(got[k], np.float64)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        assert np.isfinite(g).all(), k
        out[k] = float(np.abs(g - r).max()) / max(float(np.abs(r).max()), 1e-30)
    return out


# ------------------------------------------------------------------------------------------------------------------
# topologies
# ------------------------------------------------------------------------------------------------------------------
def _rsu(g, x, depth, mid=16, out=64):
    """RSU-<depth> block of U^2-Net: depth - 1 encoder levels joined by pooling, one dilated bottom, the decoder back up"""
    hxin = g.conv(x, out)
    hx = [g.conv(hxin, mid)]
    for _ in range(depth - 2):
        hx.append(g.conv(g.pool(hx[-1]), mid))
    d = g.conv(hx[-1], mid, dil=2)
    d = g.conv(g.concat([d, hx[-1]]), mid if depth > 2 else out)
    for lvl in range(depth - 3, -1, -1):
        up = g.interp(d, *g.shape[hx[lvl]][1:])
        d = g.conv(g.concat([up, hx[lvl]]), out if lvl == 0 else mid)
    return g.add(d, hxin)


def _rsu4f(g, x, mid=16, out=64):
    """RSU-4F: no pooling, dilations 1 2 4 8 down and 4 2 1 up"""
    hxin = g.conv(x, out)
    h1 = g.conv(hxin, mid)
    h2 = g.conv(h1, mid, dil=2)
    h3 = g.conv(h2, mid, dil=4)
    h4 = g.conv(h3, mid, dil=8)
    d3 = g.conv(g.concat([h4, h3]), mid, dil=4)
    d2 = g.conv(g.concat([d3, h2]), mid, dil=2)
    d1 = g.conv(g.concat([d2, h1]), out)
    return g.add(d1, hxin)


def u2net_small(h=384, w=384, input_name="input.1", input_params=False, out_name="1959"):
    """U^2-Net-small (the public architecture): encoders RSU7 RSU6 RSU5 RSU4 RSU4F RSU4F, decoders RSU4F RSU4 RSU5 RSU6 RSU7, six
    3x3 side outputs resized to the input, the 1x1 fusion convolution with a sigmoid, and the six side sigmoids (dead for the
    fused output).  Returns (graph, name of the fused output blob)."""
    g = Graph(3, h, w, input_name, input_params)
    e1 = _rsu(g, input_name, 7)
    e2 = _rsu(g, g.pool(e1), 6)
    e3 = _rsu(g, g.pool(e2), 5)
    e4 = _rsu(g, g.pool(e3), 4)
    e5 = _rsu4f(g, g.pool(e4))
    e6 = _rsu4f(g, g.pool(e5))

    def up_to(x, ref):
        return g.interp(x, *g.shape[ref][1:])

    d5 = _rsu4f(g, g.concat([up_to(e6, e5), e5]))
    d4 = _rsu(g, g.concat([up_to(d5, e4), e4]), 4)
    d3 = _rsu(g, g.concat([up_to(d4, e3), e3]), 5)
    d2 = _rsu(g, g.concat([up_to(d3, e2), e2]), 6)
    d1 = _rsu(g, g.concat([up_to(d2, e1), e1]), 7)
    sides = [g.conv(d1, 1, act=0)]
    for s in (d2, d3, d4, d5, e6):
        sides.append(g.interp(g.conv(s, 1, act=0), h, w))
    fused = g.conv(g.concat(sides), 1, k=1, act=4, name=out_name)
    for s in sides:
        g.sigmoid(s)
    return g, fused


def net_convs(cin, h, w, dils=(1, 2, 4, 8), couts=(64, 16, 1), out_name=None):
    """every (dilation, outputs) pair on a cin-channel input; per dilation the results are joined (an odd channel total,
    three runs) and convolved again, the four branches summed, a 1x1 sigmoid on top -- so that every layer is live"""
    g = Graph(cin, h, w)
    ys = []
    for d in dils:
        parts = [g.conv("in0", co, dil=d, act=1 if co > 1 else 0) for co in couts]
        ys.append(g.conv(g.concat(parts) if len(parts) > 1 else parts[0], 16, dil=d))
    s = ys[0]
    for y in ys[1:]:
        s = g.add(s, y)
    return g, g.conv(s, 1, k=1, act=4, name=out_name)


def net_ops(h, w):
    """pooling down to 1 x 1 (odd sizes on the way), Interp up from every level incl. the 1 x 1 one and by non-integer ratios,
    Interp down, add, Concat of 2 and of 6, pooling / Interp / Sigmoid of a Concat result, the 1x1 sigmoid layer"""
    g = Graph(3, h, w)
    c = g.conv("in0", 16)
    levels = [c]
    while g.shape[levels[-1]][1] > 1 or g.shape[levels[-1]][2] > 1:
        levels.append(g.pool(levels[-1]))
    picks = levels[1:][-5:]  # the five smallest levels, the last one 1 x 1
    sides = [g.interp(g.conv(p, 1, act=0), h, w) for p in picks]
    # non-integer ratios up and down, then back
    p2 = levels[min(2, len(levels) - 1)]
    _, h2, w2 = g.shape[p2]
    z = g.interp(g.interp(g.interp(p2, 2 * h2 + 3, 3 * w2 - 1), max(h2 - 2, 1), max(w2 - 3, 1)), h, w)
    t = g.add(z, c)
    # a Concat result read by Pooling, Interp and Sigmoid
    k2 = g.concat([t, c])
    q = g.interp(g.sigmoid(g.pool(k2)), h, w)
    sides.append(g.conv(g.conv(g.concat([q, t]), 16), 1, act=0))
    return g, g.conv(g.concat(sides), 1, k=1, act=4)


def net_thin(h=9):
    """a 1-pixel-wide input: convolution, Interp to a wider image, a live Sigmoid layer as the output"""
    g = Graph(3, h, 1)
    c = g.conv("in0", 16)
    r = g.interp(c, 2 * h + 2, 7)
    return g, g.sigmoid(g.conv(g.conv(r, 64), 1, act=0))


MODEL_STEM = "skysegsmall_sim-opt-fp16"  # the file names the reference loads (src/PatchMatch.cpp:5-6)


def write_brightness_model(folder):
    """a hand-made stand-in for the real model, under the reference's file names and blob names: p = sigmoid(3 x the 3x3 mean of the
    normalised red plane), i.e. "bright red = sky" -- a mask that follows the image content, so that the folder tests can tell
    whether masks are in use.  Returns (param path, bin path)."""
    g = Graph(3, 384, 384, "input.1", input_params=False)
    c = g.conv("input.1", 16)
    out = g.conv(c, 1, k=1, act=4, name="1959")
    w1 = np.zeros((16, 3, 3, 3), np.float32)
    w1[0, 0], w1[1, 0] = 1.0 / 9.0, -1.0 / 9.0  # relu(m) and relu(-m) of the mean m
    w2 = np.zeros(16, np.float32)
    w2[0], w2[1] = 3.0, -3.0
    weights = [(FP16_TAG, w1.reshape(-1).astype(np.float16), np.zeros(16, np.float32)), (0, w2, np.zeros(1, np.float32))]
    assert out == "1959"
    return write_pair(folder, g.emit(), stem=MODEL_STEM, weights=weights)


def smooth_image(c, h, w, seed=0):
    """a smooth image in the range of normalised pixels"""
    yy, xx = np.mgrid[0:h, 0:w]
    yy, xx = yy / max(h - 1, 1), xx / max(w - 1, 1)
    rs = np.random.RandomState(seed)
    out = np.empty((c, h, w), np.float32)
    for k in range(c):
        a, b, p = rs.uniform(1, 6, 3)
        out[k] = 1.5 * np.sin(a * xx + p) * np.cos(b * yy) + rs.uniform(-0.5, 0.5)
    return out


def noise_image(c, h, w, seed=0):
    return np.random.RandomState(seed).uniform(-2.1, 2.6, (c, h, w)).astype(np.float32)


def probe_sky_image():
    """the synthetic photo of the issue's probe: a blue gradient over textured ground, normalised -> float32 [3, 384, 384] (R,G,B)"""
    yy, xx = np.mgrid[0:384, 0:384] / 383.0
    img = np.zeros((384, 384, 3), np.float32)
    img[..., 0] = np.where(yy < 0.45, 110 + 60 * yy, 90 + 50 * np.sin(37 * xx) * np.cos(23 * yy))
    img[..., 1] = np.where(yy < 0.45, 160 + 40 * yy, 100 + 40 * np.sin(29 * xx + 1) * np.cos(31 * yy))
    img[..., 2] = np.where(yy < 0.45, 235 - 30 * yy, 70 + 60 * np.sin(41 * xx + 2) * np.cos(17 * yy))
    img = np.clip(np.rint(img + np.random.RandomState(0).normal(0, 4, img.shape)), 0, 255).astype(np.float32)
    mean = np.array([0.485, 0.456, 0.406], np.float32) * 255
    norm = 1 / np.array([0.229, 0.224, 0.225], np.float32) / 255
    return np.ascontiguousarray(((img - mean) * norm).transpose(2, 0, 1))


# ------------------------------------------------------------------------------------------------------------------
# preprocessing restated in numpy (the tests' own statement of what the device does)
# ------------------------------------------------------------------------------------------------------------------
def _reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    i = np.abs(i)
    period = 2 * (n - 1)
    i = i % period
    return np.where(i >= n, period - i, i)


def pyrdown_u8(img):
    """5x5 binomial [1 4 6 4 1]^2 / 256 around (2x, 2y), reflect-101, size (w // 2, h // 2), (s + 128) >> 8; uint8 [h, w, c]"""
    h, w = img.shape[:2]
    oh, ow = h // 2, w // 2
    k = (1, 4, 6, 4, 1)
    a = img.astype(np.int32)
    ys = _reflect101(2 * np.arange(oh)[:, None] + np.arange(-2, 3)[None, :], h)  # [oh, 5]
    xs = _reflect101(2 * np.arange(ow)[:, None] + np.arange(-2, 3)[None, :], w)
    rows = sum(k[j] * a[:, xs[:, j]] for j in range(5))  # [h, ow, c]
    s = sum(k[j] * rows[ys[:, j]] for j in range(5))  # [oh, ow, c]
    return ((s + 128) >> 8).astype(np.uint8)


def resize_linear_f32(plane, new_h, new_w):
    """the project's ResizeLinear in float32, step by step as the host states it"""
    f = np.float32
    h, w = plane.shape
    sx, sy = f(w) / f(new_w), f(h) / f(new_h)

    def axis(n_dst, scale, n_src):
        fpos = (np.arange(n_dst, dtype=f) + f(0.5)) * scale - f(0.5)
        i0 = np.floor(fpos).astype(np.int64)
        a = (fpos - i0.astype(f)).astype(f)
        lo = i0 < 0
        i0[lo], a[lo] = 0, 0
        hi = i0 >= n_src - 1
        i0[hi], a[hi] = n_src - 1, 0
        return i0, np.minimum(i0 + 1, n_src - 1), a

    y0, y1, ay = axis(new_h, sy, h)
    x0, x1, ax = axis(new_w, sx, w)
    p = plane.astype(f)
    top = p[y0][:, x0] + ax[None, :] * (p[y0][:, x1] - p[y0][:, x0])
    bot = p[y1][:, x0] + ax[None, :] * (p[y1][:, x1] - p[y1][:, x0])
    return (top + ay[:, None] * (bot - top)).astype(f)


def preprocess_u8(bgr, net_h=384, net_w=384):
    """maskExtractor's input from a uint8 [h, w, 3] B,G,R image: the pyrDown loop, the resize rounded to bytes, R,G,B planes,
    (v - mean) * norm in float32 -> float32 [3, net_h, net_w]"""
    f = np.float32
    img = np.asarray(bgr)
    while img.shape[0] > 768 and img.shape[1] > 768:
        img = pyrdown_u8(img)
    mean = [f(0.485) * f(255), f(0.456) * f(255), f(0.406) * f(255)]
    norm = [f(1) / f(0.229) / f(255), f(1) / f(0.224) / f(255), f(1) / f(0.225) / f(255)]
    out = np.empty((3, net_h, net_w), f)
    for c in range(3):
        v = np.rint(resize_linear_f32(img[:, :, 2 - c], net_h, net_w)).astype(f)
        out[c] = (v - mean[c]) * norm[c]
    return out
