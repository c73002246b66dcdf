"""The model loader of the sky-segmentation engine (mpmvs_skyseg_inspect: host code, no device) and the host statement of the
network's preprocessing, checked without a GPU."""
import os

import numpy as np
import pytest

import skyseg_common as sc


def _inspect(engine, tmp_path, layers, out=None, size=(12, 12), **kw):
    pp, bp = sc.write_pair(tmp_path, layers, **kw)
    return engine.skyseg_inspect(pp, bp, size[0], size[1], out)


def test_writer_loader_round_trip(engine, tmp_path):
    for fmt in ("fp16", "fp32", "mixed"):
        g, out = sc.net_convs(6, 37, 53)
        layers = g.emit()
        got = _inspect(engine, tmp_path, layers, out, (37, 53), fmt=fmt, seed=3)
        convs = [l for l in layers if l[0] == "Convolution"]
        blobs = set(b for l in layers for b in l[2] + l[3])
        assert got["layers"] == len(layers) and got["blobs"] == len(blobs) and got["convolutions"] == len(convs) == 17
        assert got["live_layers"] == len(layers)
        assert got["weight_bytes"] == os.path.getsize(tmp_path / "net.bin")
        assert got["macs"] == sum(l[4][6] for l in convs) * 37 * 53
    # dead layers are dropped: the six side sigmoids of the full topology
    g, out = sc.u2net_small()
    got = _inspect(engine, tmp_path, g.emit(), out, (384, 384))
    assert (got["layers"], got["blobs"], got["convolutions"], got["live_layers"]) == (331, 403, 119, 325)
    assert got["macs"] == 28448769024 and got["weight_bytes"] == 2257156
    # NULL output = the last layer's output: one of the sigmoids, which needs one side output only
    assert _inspect(engine, tmp_path, g.emit(), None, (384, 384))["live_layers"] < 325
    # pooled sizes are ceil(n / 2): the macs of a convolution after two poolings of 37 x 53
    g = sc.Graph(3, 37, 53)
    c = g.conv(g.pool(g.pool(g.conv("in0", 16))), 16)
    assert _inspect(engine, tmp_path, g.emit(), c, (37, 53))["macs"] == 16 * 3 * 9 * 37 * 53 + 16 * 16 * 9 * 10 * 14


def _small():
    g = sc.Graph(3, 12, 12)
    c = g.conv("in0", 16)
    p = g.pool(c)
    r = g.interp(p, 12, 12)
    a = g.add(r, c)
    k = g.concat([a, c])
    return g, g.conv(k, 1, k=1, act=4)


def _edit(layers, layer_type, **prm):
    """the first layer of that type with parameters changed (None removes one)"""
    out = []
    done = False
    for t, name, ins, outs, p in layers:
        p = dict(p)
        if t == layer_type and not done:
            done = True
            for k, v in prm.items():
                key = int(k[1:])
                if v is None:
                    p.pop(key, None)
                else:
                    p[key] = v
        out.append((t, name, ins, outs, p))
    assert done
    return out


DEFECTS = {
    # name: (code, editor of the emitted layer list, word the message must hold)
    "unknown_layer": (-22, lambda L: L[:2] + [("ReLU", "Relu_x", [L[1][3][0]], ["relu_out"], {})] + L[2:], "Relu_x"),
    "conv_stride": (-23, lambda L: _edit(L, "Convolution", k3=2), "Conv_c1"),
    "conv_group": (-23, lambda L: _edit(L, "Convolution", k7=2), "Conv_c1"),
    "conv_nonsquare": (-23, lambda L: _edit(L, "Convolution", k11=1), "Conv_c1"),
    "conv_5x5": (-23, lambda L: _edit(L, "Convolution", k1=5, k4=2, k6=16 * 3 * 25), "Conv_c1"),
    "conv_pad": (-23, lambda L: _edit(L, "Convolution", k4=0), "Conv_c1"),
    "conv_int8": (-24, lambda L: _edit(L, "Convolution", k8=1), "Conv_c1"),
    "pool_avg": (-25, lambda L: _edit(L, "Pooling", k0=1), "MaxPool_p2"),
    "pool_3x3": (-25, lambda L: _edit(L, "Pooling", k1=3), "MaxPool_p2"),
    "pool_stride1": (-25, lambda L: _edit(L, "Pooling", k2=1), "MaxPool_p2"),
    "interp_nearest": (-26, lambda L: _edit(L, "Interp", k0=1), "Resize_r3"),
    "interp_align_corner": (-26, lambda L: _edit(L, "Interp", k6=1), "Resize_r3"),
    "interp_by_scale": (-26, lambda L: _edit(L, "Interp", k3=None, k4=None, k1="2.0", k2="2.0"), "Resize_r3"),
    "binary_mul": (-27, lambda L: _edit(L, "BinaryOp", k0=2), "Add_a4"),
    "binary_scalar": (-27, lambda L: _edit(L, "BinaryOp", k1=1, k2="0.5"), "Add_a4"),
    "graph_does_not_close": (-31, lambda L: _edit(L, "Interp", k3=11), "Add_a4"),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_loader_rejections(engine, tmp_path, defect):
    code, edit, word = DEFECTS[defect]
    g, out = _small()
    good = g.emit()
    assert _inspect(engine, tmp_path, good, out)["layers"] == len(good)
    with pytest.raises(engine.SkySegError) as e:
        _inspect(engine, tmp_path, edit(good), out, stem=defect)
    assert e.value.code == code, (e.value.code, e.value.text)
    assert word in e.value.text, e.value.text


def test_loader_rejections_of_the_files(engine, tmp_path):
    g, out = _small()
    good = g.emit()
    pp, bp = sc.write_pair(tmp_path, good, seed=1)

    def code_of(p=pp, b=bp, o=out, size=(12, 12)):
        with pytest.raises(engine.SkySegError) as e:
            engine.skyseg_inspect(p, b, size[0], size[1], o)
        return e.value.code, e.value.text

    assert code_of(p=str(tmp_path / "missing.param"))[0] == -20
    assert code_of(b=str(tmp_path / "missing.bin"))[0] == -20
    assert code_of(o="nope") == (-32, "skyseg: no blob named nope")
    assert code_of(size=(0, 12))[0] == -2
    # wrong magic
    assert code_of(p=sc.write_pair(tmp_path, good, seed=1, stem="magic", magic="7767518")[0])[0] == -21
    # a blob read before it is written: the last two layers swapped
    swapped = good[:-2] + [good[-1], good[-2]]
    c, text = code_of(p=sc.write_pair(tmp_path, swapped, seed=1, stem="order")[0])
    assert c == -28 and good[-1][1] in text
    # layer count line that does not match
    txt = open(pp).read().split("\n")
    txt[1] = f"{len(good) + 1} 99"
    open(tmp_path / "count.param", "w").write("\n".join(txt))
    assert code_of(p=str(tmp_path / "count.param"))[0] == -21
    # weight file: too short (inside the weights, inside the last bias, before a tag), bytes left over, unknown tag
    raw = open(bp, "rb").read()
    for cut in (3, 40, len(raw) - 2, len(raw) - 12):
        open(tmp_path / "short.bin", "wb").write(raw[:cut])
        c, text = code_of(b=str(tmp_path / "short.bin"))
        assert c == -29 and "Conv_" in text, (cut, c, text)
    open(tmp_path / "long.bin", "wb").write(raw + b"\0")
    assert code_of(b=str(tmp_path / "long.bin"))[0] == -30
    open(tmp_path / "tag.bin", "wb").write(np.uint32(0x0002C056).tobytes() + raw[4:])
    c, text = code_of(b=str(tmp_path / "tag.bin"))
    assert c == -24 and "0x0002C056" in text and "Conv_c1" in text
    # all the codes above are distinct per kind of defect
    assert len({v[0] for v in DEFECTS.values()} | {-20, -21, -28, -29, -30, -32}) == 13


def test_both_weight_tags_are_read(engine, tmp_path):
    """tag 0x01306B47 (halfs, padded to 4 bytes) and tag 0 (raw fp32) are both accepted and consume their own byte counts (the
    values are compared on the GPU, where the nets run)"""
    g, out = _small()
    layers = g.emit()
    a = _inspect(engine, tmp_path, layers, out, fmt="fp16", seed=5, stem="h")
    b = _inspect(engine, tmp_path, layers, out, fmt="fp32", seed=5, stem="f")
    n = sum(l[4][6] for l in layers if l[0] == "Convolution")
    assert b["weight_bytes"] - a["weight_bytes"] == 4 * n - sum((2 * l[4][6] + 3) // 4 * 4 for l in layers if l[0] == "Convolution")


@pytest.mark.parametrize("size", [(384, 384), (500, 700), (770, 1000), (1540, 1538), (769, 3100), (37, 53)])
def test_host_preprocessing_against_numpy(hostlib, size):
    """pyrDown loop / resize / normalise as the host states them == the numpy restatement of skyseg_common, bit for bit"""
    h, w = size
    rs = np.random.RandomState(w)
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    img[: h // 3] = (img[: h // 3] // 8 + np.array([200, 150, 90])).astype(np.uint8)   # a flat "sky" band
    assert np.array_equal(hostlib.sky_preprocess(img), sc.preprocess_u8(img))
    if h >= 2 and w >= 2:
        assert np.array_equal(hostlib.pyrdown8(img), sc.pyrdown_u8(img))
        assert np.array_equal(hostlib.pyrdown8(img[:, :, 0]), sc.pyrdown_u8(img[:, :, :1])[:, :, 0])


def test_pyrdown_is_the_binomial_filter(hostlib):
    """independent of both restatements: a constant image stays constant, an impulse spreads as [1 4 6 4 1]^2 / 256 sampled at even
    pixels, and the border reflects without repeating the edge pixel"""
    assert (hostlib.pyrdown8(np.full((9, 10), 77, np.uint8)) == 77).all()
    im = np.zeros((12, 12), np.uint8)
    im[6, 6] = 255
    out = hostlib.pyrdown8(im).astype(int)
    k = np.array([1, 4, 6, 4, 1])
    want = (255 * np.outer(k, k)[::2, ::2] + 128) >> 8
    assert np.array_equal(out[2:5, 2:5], want) and out.sum() == want.sum()
    row = np.zeros((2, 8), np.uint8)
    row[:, 1] = 160   # reflect-101 at x = -1 reads x = 1, at x = -2 reads x = 2
    assert hostlib.pyrdown8(row)[0, 0] == ((4 + 4) * 160 * 16 + 128) >> 8


def test_real_model_when_given(engine):
    """with MPMVS_SKY_MODEL naming the directory of the real pair: its counts, and the topology builder emits its layer list"""
    d = os.environ.get("MPMVS_SKY_MODEL")
    if not d:
        pytest.skip("MPMVS_SKY_MODEL is not set")
    pp, bp = os.path.join(d, "skysegsmall_sim-opt-fp16.param"), os.path.join(d, "skysegsmall_sim-opt-fp16.bin")
    got = engine.skyseg_inspect(pp, bp, 384, 384, "1959")
    assert got == dict(layers=331, blobs=403, convolutions=119, live_layers=325, weight_bytes=2257156, macs=28448769024)
    assert os.path.getsize(bp) == 2257156
    with pytest.raises(engine.SkySegError) as e:
        engine.skyseg_inspect(pp, bp, 380, 384, "1959")   # the graph only closes for 384 x 384
    assert e.value.code == -31
    nl, nb, real = sc.read_param(pp)
    g, out = sc.u2net_small()
    mine = g.emit()
    assert (nl, nb) == (331, 403) and out == "1959"
    assert sc.canonical(mine) == sc.canonical(real)
    assert [l[3] for l in mine if l[0] == "Input"] == [["input.1"]] and real[-7][3] == ["1959"]
