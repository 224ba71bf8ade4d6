"""What the label drawing costs on the host, in the cases tools/detect_path.py does not time:

* `pillow_draw`: the whole /detect request of tools/detect_path.py with the drop-in's `Image` (GPU decode / encode)
  but Pillow's own `PIL.ImageDraw` — a caller that draws with plain Pillow on a GPU-decoded image, so the image's
  host pixels are made on demand (DeviceRGBImage.load) and uploaded again by save. Same stages as detect_path.
* `load_ms_p50`: DeviceRGBImage.load() alone on the fixture (device idle before the call).
* `draw_host_ms`: the 16 labels of one request (fixed boxes, serve.py's calls) drawn through the drop-in's
  ImageDraw on a GPU-decoded image without flushing (`record`), and through Pillow's ImageDraw with a core object
  that does nothing (`pillow_python`: colour parsing, text layout, the memoised masks); the difference per label
  is the recorder. Only with a package that has the device draw.

    python tools/draw_host_copy.py [--iters 200] [--tree DIR]

--tree DIR: import spotter_amd and tools/detect_path.py from DIR (a checkout of another commit) instead of this tree.
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    root = os.path.abspath(a.tree)
    sys.path.insert(0, os.path.join(root, "tools"))
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from PIL import Image as PILImage
    from PIL import ImageDraw as PILDraw

    import detect_path
    from spotter_amd import draw as sdraw
    from spotter_amd.jpeg import image_module, open_image

    def opener(decode):
        Image = image_module()
        return (lambda data: Image.open(io.BytesIO(data))), PILDraw

    detect_path.opener = opener
    out = {"pillow_draw": detect_path.measure("r101vd", a.iters, decode="gpu", jitter=False)}
    out["pillow_draw"].pop("metric", None)

    with open(os.path.join(root, "tests", "golden", "test_pic.jpg"), "rb") as f:
        data = f.read()
    ts = []
    for _ in range(60):
        im = open_image(data).convert("RGB")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        im.load()
        ts.append((time.perf_counter() - t0) * 1e3)
    out["load_ms_p50"] = round(float(np.percentile(ts[10:], 50)), 3)

    if hasattr(sdraw, "DeviceDraw"):
        rng = np.random.default_rng(16)
        texts = sorted(set(detect_path.AMENITIES.values()))
        labels = []
        for i in range(16):
            x0, y0 = rng.uniform(0, 1100), rng.uniform(0, 650)
            labels.append(([x0, y0, x0 + rng.uniform(20, 500), y0 + rng.uniform(20, 400)], texts[i % len(texts)]))

        def draw_all(d):
            for box, text in labels:
                d.rectangle(box, outline="red", width=3)
                d.text(xy=(box[0] + 5, box[1] + 5), text=text, fill="white", stroke_width=1, stroke_fill="black")

        class Nothing:
            draw_ink = staticmethod(lambda color: -1 if color in (-1, (255, 255, 255)) else 255)

            def draw_rectangle(self, *args):
                pass

            def draw_bitmap(self, *args):
                pass

        shim = sdraw.draw_module()
        dev_im = open_image(data).convert("RGB")
        host_im = PILImage.new("RGB", dev_im.size)
        best = {"record": 1e9, "pillow_python": 1e9}
        for _ in range(40):
            for name in best:
                t0 = time.perf_counter()
                for _ in range(10):
                    if name == "record":
                        d = shim.Draw(dev_im)
                        assert type(d) is sdraw.DeviceDraw
                        draw_all(d)
                        dev_im._draw_list.clear()
                    else:
                        d = shim.Draw(host_im)
                        d.draw = Nothing()
                        draw_all(d)
                best[name] = min(best[name], (time.perf_counter() - t0) / 10 * 1e3)
        out["draw_host_ms"] = {k: round(v, 4) for k, v in best.items()}
        out["recorder_us_per_label"] = round((best["record"] - best["pillow_python"]) / 16 * 1e3, 2)
        out["draw_host_note"] = "best of 40 rounds of 10 draws of 16 labels, masks memoised"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
