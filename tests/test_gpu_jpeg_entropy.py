"""GPU: the entropy decode of baseline JPEGs on the device (JpegDecoder(entropy="gpu"): sp_jpeg_entropy_pack on the
host, sp_jpeg_entropy_decode + the unchanged sp_jpeg_to_rgb on the GPU) against the host entropy decoder's
coefficients and Pillow's pixels, bit for bit; which path ran is read from decoder.stats. The inputs are
tests/jpeg_entropy_cases.py's, the ones the CPU emulation of the same code runs in tests/test_jpeg_entropy_host.py."""
import io
import os
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from PIL import Image  # noqa: E402

sys.path.insert(0, os.path.dirname(__file__))
from jpeg_entropy_cases import cases, non_eligible, resistant, tail_junk  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    from spotter_amd._lib import lib

    assert lib().sp_device_init(0) == 0, lib().sp_last_error()
    return torch.device("cuda", 0)


def _pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _device_coefs(d, lay):
    return d._g["coefs"][:lay.total_blocks * 64].cpu().numpy().reshape(-1, 64)


def test_gpu_entropy_matches_host_coefficients(dev):
    from spotter_amd.jpeg import JpegDecoder, decode_coefs

    d = JpegDecoder(dev, entropy="gpu")
    n = 0
    for name, data in cases():
        got = d.decode(data).cpu().numpy()
        lay, ref_co = decode_coefs(data)
        assert d.stats["gpu"] == n + 1 and not d.stats["fallback"] and d.stats["host"] == 0, (name, d.stats)
        co = _device_coefs(d, lay)
        bad = np.argwhere(co != ref_co)
        assert bad.size == 0, f"{name}: {len(bad)} coefficients differ, first at {bad[:3].tolist()}"
        ref = _pillow(data)
        assert got.shape == ref.shape, name
        bad = np.argwhere(got != ref)
        assert bad.size == 0, f"{name}: {len(bad)} samples differ, first at {bad[:3].tolist()}"
        n += 1
    assert n >= 25 and d.stats["gpu"] == n and d.stats["fallback"] == {}


def test_sync_resistant_streams_give_pillows_pixels(dev):
    """Flat frames, 8-pixel-periodic stripes, an all-black 640x480: the pixels are Pillow's, by whichever path."""
    from spotter_amd.jpeg import JpegDecoder

    d = JpegDecoder(dev, entropy="auto")
    for name, data in resistant():
        got = d.decode(data).cpu().numpy()
        assert np.array_equal(got, _pillow(data)), name
    assert d.stats["gpu"] + sum(d.stats["fallback"].values()) == len(resistant()) and d.stats["host"] == 0


def test_non_eligible_files_take_the_host_path(dev):
    from spotter_amd.jpeg import JpegDecoder

    d, h = JpegDecoder(dev, entropy="gpu"), JpegDecoder(dev)
    for k, (name, data) in enumerate(non_eligible()):
        got = d.decode(data)
        assert d.stats["host"] == k + 1 and d.stats["gpu"] == 0 and not d.stats["fallback"], (name, d.stats)
        assert torch.equal(got, h.decode(data)), name
        assert np.array_equal(got.cpu().numpy(), _pillow(data)), name
    assert h.stats == {"gpu": 0, "host": 0, "fallback": {}, "h2d_bytes": 0}  # the default path counts nothing


def test_gpu_entropy_on_the_corrupt_corpus(dev, monkeypatch):
    """tests/jpeg_corpus.py through the drop-in Image.open with SPOTTER_JPEG_ENTROPY=gpu, the three-way rule of
    test_gpu_jpeg.py::test_gpu_path_on_the_corrupt_corpus: GPU-decoded with Pillow's pixels, or Pillow's own image
    object, or Pillow's exception — and for every file the outcome a default decoder gives for the same bytes."""
    from jpeg_corpus import corpus

    from spotter_amd import jpeg
    from spotter_amd.jpeg import DeviceRGBImage, JpegDecoder, UnsupportedJpeg

    monkeypatch.setenv("SPOTTER_JPEG_ENTROPY", "gpu")
    monkeypatch.setattr(jpeg, "_decoders", {})
    shim = jpeg.image_module(dev)
    assert shim._spotter_entropy == "gpu"
    host = JpegDecoder(dev)
    gpu = declined = 0
    for lab, data in list(corpus()) + list(tail_junk()):
        try:
            want = host.decode(data)
        except UnsupportedJpeg:
            want = None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                ref_im = Image.open(io.BytesIO(data))
            except Exception as e:  # noqa: BLE001 - whatever Pillow raises, the shim raises too
                with pytest.raises(type(e)):
                    shim.open(io.BytesIO(data))
                continue
            im = shim.open(io.BytesIO(data))
            if isinstance(im, DeviceRGBImage):
                gpu += 1
                assert want is not None and type(ref_im).__name__ == "JpegImageFile" and ref_im.mode == "RGB", lab
                assert torch.equal(im.spotter_device_rgb, want), lab
                assert np.array_equal(np.asarray(im.convert("RGB")), np.asarray(ref_im.convert("RGB"))), lab
            else:
                declined += 1
                assert type(im) is type(ref_im), lab
                assert want is None or ref_im.mode != "RGB", lab
    stats = jpeg.decoder(dev, "gpu").stats
    assert gpu >= 100 and declined >= 100, (gpu, declined)
    assert stats["gpu"] >= 50 and stats["host"] >= 50 and sum(stats["fallback"].values()) >= 10, stats


def test_extra_bytes_after_the_last_block_fall_back(dev):
    """Eligible files (gray ones too, which the drop-in leaves to Pillow) with 1..48 extra bytes before EOI or a
    restart marker, straight through the decoders: never the GPU path's result, always what the default decoder
    gives — its pixels, or its UnsupportedJpeg."""
    from spotter_amd.jpeg import JpegDecoder, UnsupportedJpeg

    d, h = JpegDecoder(dev, entropy="gpu"), JpegDecoder(dev)
    refused = 0
    for lab, data in tail_junk():
        try:
            want = h.decode(data)
        except UnsupportedJpeg:
            want = None
        if want is None:
            refused += 1
            with pytest.raises(UnsupportedJpeg):
                d.decode(data)
        else:
            assert torch.equal(d.decode(data), want), lab
    assert d.stats["gpu"] == 0 and d.stats["host"] == 0 and sum(d.stats["fallback"].values()) == len(tail_junk())
    assert refused >= 200


def test_two_decoders_on_two_streams(dev):
    """Two decoders, each on its own torch stream, decode different files alternately with nothing between them
    but the streams' own order: the results equal the single-stream ones."""
    from spotter_amd.jpeg import JpegDecoder

    files = [data for name, data in cases() if name in ("480x640 sub0", "233x177 sub2", "test_pic baseline",
                                                         "restart rows", "noise q100", "gray 233x177")]
    assert len(files) == 6
    single = JpegDecoder(dev, entropy="gpu")
    want = [single.decode(f).clone() for f in files]
    torch.cuda.synchronize(dev)
    decs = [JpegDecoder(dev, entropy="gpu"), JpegDecoder(dev, entropy="gpu")]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    got = {}
    for rep in range(2):
        for k, f in enumerate(files):
            w = (k + rep) % 2
            with torch.cuda.stream(streams[w]):
                got[(rep, k)] = decs[w].decode(f)
    torch.cuda.synchronize(dev)
    for (rep, k), t in got.items():
        assert torch.equal(t, want[k]), (rep, k)
    assert decs[0].stats["gpu"] + decs[1].stats["gpu"] == 12


def test_drop_in_with_the_environment_variable(dev, monkeypatch):
    """SPOTTER_JPEG_ENTROPY=gpu in a fresh image_module: processor(images=Image.open(bytes)) is bit-equal to the
    Pillow route for a baseline 4:2:0 file, and the GPU entropy path ran."""
    from spotter_amd import SpotterImageProcessor, jpeg
    from spotter_amd.jpeg import DeviceRGBImage

    monkeypatch.setenv("SPOTTER_JPEG_ENTROPY", "gpu")
    monkeypatch.setattr(jpeg, "_decoders", {})
    monkeypatch.setattr(jpeg, "_env_entropy", None)  # open_image reads the variable once per process
    Img = jpeg.image_module(dev)
    data = dict(cases())["test_pic baseline"]
    proc = SpotterImageProcessor()
    with Img.open(io.BytesIO(data)) as raw:
        im = raw.convert("RGB")
        assert isinstance(im, DeviceRGBImage)
        a = proc(images=im)["pixel_values"]
    b = proc(images=Image.open(io.BytesIO(data)).convert("RGB"))["pixel_values"]
    assert torch.equal(a, b)
    assert jpeg.decoder(dev, "gpu").stats["gpu"] == 1 and jpeg.decoder(dev, "gpu").entropy == "gpu"
    with jpeg.open_image(data, dev) as raw:  # open_image reads the same default
        assert torch.equal(proc(images=raw.convert("RGB"))["pixel_values"], b)
    assert jpeg.decoder(dev, "gpu").stats["gpu"] == 2
    monkeypatch.setenv("SPOTTER_JPEG_ENTROPY", "host")  # latched: neither the module nor open_image re-reads it
    with Img.open(io.BytesIO(data)) as raw, jpeg.open_image(data, dev) as raw2:
        assert isinstance(raw, DeviceRGBImage) and isinstance(raw2, DeviceRGBImage)
    assert jpeg.decoder(dev, "gpu").stats["gpu"] == 4
