"""The device PNG encoder on the GPU (csrc/png_encode.hip, relightable3dgaussian_amd/png_device.py, FrameWriter(device_png=True),
--device_png): png_device.encode gives, byte for byte and with the same count, the stream of tests/png_reference.zlib_stream for
every picture of tests/png_cases.py and both tables; no share of the bytes is left out.  The picture sits 1 byte off its
allocation's alignment; 64-byte canaries stand on both sides of the stream buffer and of the scratch, and every byte past the
returned count is as it was.  Then the refusals, the writer against the PIL writer, and the two drivers with the flag."""
import os

import numpy as np
import pytest
import torch

from tests import png_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 0xA5


def _tables():
    from relightable3dgaussian_amd import png_device
    return {"default": png_device.DEFAULT_TABLE, "fixed": png_device.FIXED_TABLE}


def _off_by_one(x):
    flat = torch.empty(x.size + 1, dtype=torch.uint8, device=DEV)
    flat[1:] = torch.from_numpy(np.array(x)).reshape(-1).to(DEV)
    t = flat[1:].reshape(x.shape)
    assert t.data_ptr() % 16 == 1
    return t


def _raw_encode(x_dev, table, W, H, C, capacity=None, header_bits=None, shape=None):
    """r3dg_png_encode itself on guarded buffers -> (status, stream buffer with canaries, scratch buffer with canaries, count, sizes)."""
    from relightable3dgaussian_amd import _lib, png_device
    L = _lib.lib()
    bound = png_device.zlib_bound(*(shape or (W, H, C)))
    nscratch = int(L.r3dg_png_scratch_bytes(*(shape or (W, H, C))))
    assert nscratch > 0
    zbuf = torch.full((bound + 128,), FILL, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((nscratch + 128,), FILL, dtype=torch.uint8, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    code_table, block_header = table.resident(torch.device(DEV, torch.cuda.current_device()))
    status = L.r3dg_png_encode(_lib.current_stream(), W, H, C, x_dev.data_ptr(), code_table.data_ptr(), block_header.data_ptr(),
                               table.header_bits if header_bits is None else header_bits, sbuf.data_ptr() + 64, nscratch,
                               zbuf.data_ptr() + 64, bound if capacity is None else capacity, count.data_ptr())
    torch.cuda.synchronize()
    return status, zbuf.cpu().numpy(), sbuf.cpu().numpy(), int(count.item()), (bound, nscratch)


@pytest.mark.parametrize("table", ["default", "fixed"])
@pytest.mark.parametrize("name", png_cases.NAMES)
def test_stream_is_the_reference_stream(name, table):
    from relightable3dgaussian_amd import _lib, png_device
    x = png_cases.picture(name)
    H, W, C = x.shape
    t = _tables()[table]
    want, stored = png_cases.reference_stream(name, table, t)
    assert _lib.lib().r3dg_png_zlib_bound(W, H, C) == png_device.zlib_bound(W, H, C)
    status, z, s, count, (bound, nscratch) = _raw_encode(_off_by_one(x), t, W, H, C)
    assert status == 0
    print("%s/%s: %d bytes raw, %d in the stream (bound %d), %d of %d segments stored"
          % (name, table, x.size, count, bound, sum(stored), len(stored)))
    assert count == len(want)
    got = z[64:64 + count].tobytes()
    if got != want:
        first = next(i for i in range(count) if got[i] != want[i])
        raise AssertionError("the stream differs from the reference from byte %d of %d on" % (first, count))
    assert (z[:64] == FILL).all() and (z[64 + count:] == FILL).all(), "bytes outside the stream were written"
    assert (s[:64] == FILL).all() and (s[64 + nscratch:] == FILL).all(), "bytes outside the scratch were written"
    # the public call: the same stream into buffers of its own
    zlib_dev, n_dev = png_device.encode(torch.from_numpy(np.array(x)).to(DEV), t)
    assert zlib_dev.numel() == bound and zlib_dev[:int(n_dev.item())].cpu().numpy().tobytes() == want


def test_rejections_leave_the_stream_untouched():
    from relightable3dgaussian_amd import _lib
    L = _lib.lib()
    t = _tables()["default"]
    x = _off_by_one(png_cases.picture("13x11x3"))
    wide = torch.zeros(65535, dtype=torch.uint8, device=DEV)
    from relightable3dgaussian_amd import png_device
    bound = png_device.zlib_bound(11, 13, 3)
    for what, kw in (("channels 0", dict(W=11, H=13, C=0)), ("channels 5", dict(W=11, H=13, C=5)),
                     ("row_bytes 65536", dict(W=65535, H=1, C=1, x=wide)), ("a capacity one byte short", dict(capacity=bound - 1)),
                     ("header_bits 0", dict(header_bits=0))):
        src = kw.pop("x", x)
        args = dict(W=11, H=13, C=3, shape=(11, 13, 3))
        args.update(kw)
        status, z, s, count, _ = _raw_encode(src, t, **args)
        assert status == -1, what
        assert (z == FILL).all() and (s == FILL).all() and count == -7, what
        assert L.r3dg_last_error(), what
    assert L.r3dg_png_zlib_bound(65535, 1, 1) < 0 and L.r3dg_png_scratch_bytes(11, 13, 5) < 0
    status = L.r3dg_png_encode(None, 11, 13, 3, None, None, None, t.header_bits, None, 0, None, 0, None)
    assert status == -1


def _pixels(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.mode, np.asarray(im)


def test_writer_gives_the_pictures_of_the_pil_writer(tmp_path):
    from relightable3dgaussian_amd.relighting import FrameWriter
    g = torch.Generator().manual_seed(4)
    image = torch.rand(3, 37, 50, generator=g) * 1.6 - 0.3               # values outside [0,1]
    image[:, 5, 7] = float("nan")
    image[1, 20:30, 10:40] = 0.5
    image = image.to(DEV)
    sheet = torch.from_numpy(png_cases.picture("13x11x3").copy()).to(DEV)
    grey = torch.rand(1, 9, 14, generator=g).to(DEV)
    for name, writer in (("pil", FrameWriter(workers=2)), ("device", FrameWriter(workers=2, slots=2, device_png=True))):
        d = tmp_path / name
        d.mkdir()
        for k in range(3):                                               # (more frames than slots: the ring comes round)
            writer.submit(image * (1.0 - 0.1 * k), str(d / ("image%d.png" % k)))
        writer.submit_bytes(sheet, str(d / "sheet.png"))
        writer.submit(grey, str(d / "grey.png"))
        writer.close()
    names = sorted(os.listdir(tmp_path / "pil"))
    assert names == sorted(os.listdir(tmp_path / "device")) == ["grey.png", "image0.png", "image1.png", "image2.png", "sheet.png"]
    for n in names:
        mode_a, a = _pixels(tmp_path / "pil" / n)
        mode_b, b = _pixels(tmp_path / "device" / n)
        assert mode_a == mode_b and a.shape == b.shape and np.array_equal(a, b), n
    assert np.array_equal(_pixels(tmp_path / "device" / "sheet.png")[1], png_cases.picture("13x11x3"))


def test_writer_raises_a_workers_error_at_close(tmp_path):
    from relightable3dgaussian_amd.relighting import FrameWriter
    writer = FrameWriter(workers=1, device_png=True)
    writer.submit(torch.zeros(3, 4, 5, device=DEV), str(tmp_path / "no" / "such" / "directory" / "frame.png"))
    with pytest.raises(OSError):
        writer.close()


from tests.test_relighting_driver_gpu import config  # noqa: E402,F401  (the fixture: the smallest scene of that file)


def test_relighting_driver_with_device_png(config):  # noqa: F811
    from relightable3dgaussian_amd import relighting
    from tests.test_relighting_driver_gpu import CAPTURES, K
    outs = {}
    for name, flag in (("pil", []), ("device", ["--device_png"])):
        outs[name] = str(config.root / ("png_" + name))
        assert relighting.main(["-co", config.cfg, "-e", config.env, "--output", outs[name], "--capture_list", ",".join(CAPTURES),
                                "--sample_num", str(K), "-bg", "0.25"] + flag) == 0
    for c in CAPTURES:
        files = sorted(os.listdir(os.path.join(outs["pil"], c)))
        assert files == sorted(os.listdir(os.path.join(outs["device"], c))) == ["frame_%s.png" % k for k in config.keys]
        for f in files:
            (ma, a), (mb, b) = _pixels(os.path.join(outs["pil"], c, f)), _pixels(os.path.join(outs["device"], c, f))
            assert ma == mb and np.array_equal(a, b), (c, f)
    assert sorted(os.listdir(outs["pil"])) == sorted(os.listdir(outs["device"]))


def test_training_driver_with_device_png(tmp_path, monkeypatch):
    """The smallest scene of tests/test_training_vis_gpu.py's driver test, stage 1, with and without the flag: the same file set,
    and every file of the --device_png run decodes to the pixels the PIL writer's file holds for the very sheet that run handed
    over (two training runs are not promised to repeat bit for bit, so the sheets are caught where the run submits them)."""
    from relightable3dgaussian_amd import dataset, relighting, training
    from tests.test_dataset_cpu import write_split
    from tests.test_dataset_gpu import _teacher_views
    cams, arrays = _teacher_views(4, 48)
    root = str(tmp_path / "data")
    os.makedirs(root)
    c2w = []
    for cam in cams:
        mat = torch.linalg.inv(cam.world_view_transform.double().t())
        mat[:3, 1:3] *= -1
        c2w.append(mat.numpy())
    write_split(root, "train", np.stack(arrays), np.stack(c2w), cams[0].FoVx)
    rng = np.random.RandomState(2)
    dataset.write_points_ply(os.path.join(root, "points3d.ply"), rng.random_sample((3000, 3)) * 2.6 - 1.3,
                             rng.random_sample((3000, 3)) * 255, np.zeros((3000, 3)))
    parse = training.build_parser().parse_args
    base = ["-s", root, "-t", "render", "-w", "--iterations", "3", "--log_interval", "0", "--seed", "3", "--save_training_vis",
            "--save_training_vis_iteration", "2"]
    submitted, modes = {}, []
    plain_submit = relighting.FrameWriter.submit_bytes

    def spy(self, bytes_dev, path):
        submitted[os.path.basename(path)] = bytes_dev.clone()
        modes.append(self.device_png)
        return plain_submit(self, bytes_dev, path)
    monkeypatch.setattr(relighting.FrameWriter, "submit_bytes", spy)
    outs = {}
    for name, flag in (("pil", []), ("device", ["--device_png"])):
        outs[name] = str(tmp_path / name)
        training.train(parse(base + ["-m", outs[name]] + flag))
    monkeypatch.undo()
    assert modes == [False, False, True, True]
    files = sorted(os.listdir(os.path.join(outs["pil"], "visualize")))
    assert files == sorted(os.listdir(os.path.join(outs["device"], "visualize"))) == ["000001.png", "000002.png"]
    writer = relighting.FrameWriter(workers=1)
    for f in files:
        writer.submit_bytes(submitted[f], str(tmp_path / ("pil_" + f)))
    writer.close()
    for f in files:
        (ma, a), (mb, b) = _pixels(str(tmp_path / ("pil_" + f))), _pixels(os.path.join(outs["device"], "visualize", f))
        assert ma == mb == "RGB" and a.any() and np.array_equal(a, b), f
        assert np.array_equal(b, submitted[f].cpu().numpy())
        assert _pixels(os.path.join(outs["pil"], "visualize", f))[1].shape == b.shape
