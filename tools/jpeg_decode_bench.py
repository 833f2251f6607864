"""Time the LLFF image path on one synthetic 4032 x 3024 4:2:0 JPEG (a real LLFF frame's size): the host stages (marker parse,
entropy decode), the copy to the device, the two decode kernels and the Lanczos resize to 504 x 378 + ToTensor — against the
reference's own path on the same box, `Image.open().convert('RGB').resize(LANCZOS)` and /255 on one CPU thread.  Not a test;
gates nothing.

    python tools/jpeg_decode_bench.py [--out profiles/jpeg_decode_bench.json] [--reps 10] [--quality 90]
    python tools/jpeg_decode_bench.py --entropy-out profiles/jpeg_entropy_bench.json      # also the entropy stage on the device

Kernel times are hipEvent intervals around each operator call, the median of --reps runs after two warm-up runs; the achieved
GB/s relate them to the kernels' algorithmic bytes (csrc/jpeg.hip).  The decode operator launches both kernels; to time them
apart the 1-component form of the same call is timed as well (inverse DCT of the luma plane + the grey write).

With --entropy-out the same file's scan is also Huffman-decoded on the device (csrc/jpeg_entropy.hip) for subseq_bits in 256, 512,
1024, 2048 and 4096: hipEvent intervals around the launches of nerfhip_jpeg_entropy_sync (prepare, the passes inside the
workgroups and the rounds between them that this file needs, found beforehand) and of nerfhip_jpeg_entropy_emit (with the zeroing
of the coefficient tensors), buffers allocated and the scan uploaded outside the interval; the rounds each setting needed; the
host-to-device bytes of both paths; and whether the coefficients equal the host decoder's."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, w, h = 4032, 3024, 504, 378


def synthetic_jpeg(quality):
    from PIL import Image
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([(x * 255) // (W - 1), (y * 255) // (H - 1), ((x + y) // 8) % 256], -1).astype(np.int16)
    img += rng.integers(-12, 13, img.shape, dtype=np.int16)                       # sensor-like noise: a photo's bit rate, not a ramp's
    img[1000:2000, 1500:2500] = rng.integers(0, 256, (1000, 1000, 3))
    buf = io.BytesIO()
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8), "RGB").save(buf, "JPEG", quality=quality, subsampling=2)
    return buf.getvalue()


def host_ms(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), r


def device_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), r


def device_entropy(parsed, coef, dev, reps, host_entropy_ms, h2d_bytes_host):
    """the device entropy stage on one file, per subseq_bits"""
    import ctypes
    from nerf_pl_amd import _lib, ops
    lib = _lib.load()
    res = {"host_entropy_ms": host_entropy_ms, "h2d_bytes_host_path": h2d_bytes_host, "sweep": []}
    for bits in (256, 512, 1024, 2048, 4096):
        got, rounds = ops.jpeg_entropy_decode_batch([parsed], dev, bits, return_rounds=True)
        equal = all(np.array_equal(g[0].cpu().numpy(), c) for g, c in zip(got, coef))
        arrays = ops._jpeg_batch_arrays("bench", [parsed], bits)
        up = [torch.from_numpy(a.copy()).to(dev) for a in arrays[:5]]
        res["h2d_bytes_device_path"] = sum(t.numel() * t.element_size() for t in up)
        nbytes = lib.nerfhip_jpeg_entropy_workspace_bytes(1, arrays[7], arrays[8], bits)
        wgs = lib.nerfhip_jpeg_entropy_workgroups(arrays[7], arrays[8], bits)
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        flags = torch.zeros(2, device=dev, dtype=torch.int32)
        b = ops._jpeg_batch_struct(ops.ptr, tuple(up) + arrays[5:], bits, ws, flags, flags[1:])
        b.status, b.progress = flags.data_ptr(), flags.data_ptr() + 4

        def sync():
            ops.check(lib.nerfhip_jpeg_entropy_sync(ctypes.addressof(b), min(rounds, 64), ops.stream_ptr()), "sync")
            done = min(rounds, 64)
            while done < rounds:
                more = min(64, rounds - done)
                ops.check(lib.nerfhip_jpeg_entropy_rounds(ctypes.addressof(b), done + 1, more, ops.stream_ptr()), "rounds")
                done += more

        def emit():
            for g in got:
                g.zero_()
            ops.check(lib.nerfhip_jpeg_entropy_emit(ctypes.addressof(b), *[ops.ptr(got[c]) if c < len(got) else None for c in range(3)],
                                                    ops.stream_ptr()), "emit")
        sync_ms, _ = device_ms(sync, reps)
        emit_ms, _ = device_ms(emit, reps)
        host = flags.cpu().numpy()
        equal = equal and host[0] == 0 and host[1] < max(rounds, 1) and all(np.array_equal(g[0].cpu().numpy(), c) for g, c in zip(got, coef))
        res["sweep"].append({"subseq_bits": bits, "workgroups": wgs, "rounds_between_workgroups": rounds, "sync_ms": sync_ms,
                             "emit_ms": emit_ms, "device_entropy_ms": sync_ms + emit_ms, "workspace_bytes": nbytes,
                             "equals_host_decoder": bool(equal)})
    best = min(res["sweep"], key=lambda r: r["device_entropy_ms"])
    res["fastest_subseq_bits"] = best["subseq_bits"]
    res["device_over_host"] = best["device_entropy_ms"] / host_entropy_ms
    return res


def _rounded(x):
    if isinstance(x, float):
        return round(x, 4)
    if isinstance(x, dict):
        return {k: _rounded(v) for k, v in x.items()}
    if isinstance(x, list):
        return [_rounded(v) for v in x]
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entropy-out", default=None, help="also time the entropy stage on the device; its JSON goes here")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quality", type=int, default=90)
    args = ap.parse_args()
    from PIL import Image
    from nerf_pl_amd import ops
    from nerf_pl_amd.imageio_min import jpeg_parse
    dev = torch.device("cuda:0")
    data = synthetic_jpeg(args.quality)
    res = {"image": "%d x %d 4:2:0 q%d, %d bytes" % (W, H, args.quality, len(data)), "resize_to": [w, h], "reps": args.reps,
           "device": torch.cuda.get_device_name(0)}

    torch.set_num_threads(1)

    def pil_path():
        img = Image.open(io.BytesIO(data)).convert("RGB").resize((w, h), Image.LANCZOS)
        return torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    res["pil_ms"], ref = host_ms(pil_path, max(3, args.reps // 2))
    t, _ = host_ms(lambda: Image.open(io.BytesIO(data)).convert("RGB"), max(3, args.reps // 2))
    res["pil_decode_only_ms"] = t

    res["parse_ms"], parsed = host_ms(lambda: jpeg_parse(data), args.reps)
    res["entropy_ms"], coef = host_ms(lambda: ops.jpeg_entropy_decode(parsed), max(3, args.reps // 2))
    comps = parsed["components"]
    quant = np.stack([parsed["quant"][c[3]] for c in comps]).astype(np.int16)
    pinned = [torch.from_numpy(c.reshape(1, -1, 64)).pin_memory() for c in coef]
    res["h2d_ms"], dcoef = device_ms(lambda: [p.to(dev, non_blocking=True) for p in pinned], args.reps)
    res["h2d_bytes"] = sum(p.numel() * 2 for p in pinned)
    dq = torch.from_numpy(quant[None]).to(dev)

    res["decode_ms"], rgbx = device_ms(lambda: ops.decode_jpeg_batch(dcoef, dq, H, W, 2, 2), args.reps)
    res["decode_grey_ms"], _ = device_ms(lambda: ops.decode_jpeg_batch(dcoef[:1], dq[:, :1].contiguous(), H, W, 1, 1), args.reps)
    blocks = sum(p.shape[1] for p in pinned)
    res["idct_bytes"] = blocks * 64 * 3                      # 2 B/coefficient in, 1 B/sample out
    res["rgbx_bytes"] = blocks * 64 + W * H * 4              # planes in, 4 B/pixel out
    res["decode_gbps"] = (res["idct_bytes"] + res["rgbx_bytes"]) / res["decode_ms"] / 1e6
    res["resize_ms"], small = device_ms(lambda: ops.resize_rgba_lanczos(rgbx, w, h), args.reps)
    res["to_float_ms"], out = device_ms(lambda: ops.rgba_to_rgb_white(small)[0], args.reps)
    got = out.reshape(h, w, 3).permute(2, 0, 1).cpu()
    res["equals_pil"] = bool(torch.equal(got, ref))
    res["ours_ms"] = sum(res[k] for k in ("parse_ms", "entropy_ms", "h2d_ms", "decode_ms", "resize_ms", "to_float_ms"))
    res["device_ms"] = sum(res[k] for k in ("decode_ms", "resize_ms", "to_float_ms"))
    res["speedup_vs_pil"] = res["pil_ms"] / res["ours_ms"]
    res["host_share"] = (res["parse_ms"] + res["entropy_ms"]) / res["ours_ms"]
    line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()})
    print(line)
    if args.entropy_out:
        ent = device_entropy(parsed, coef, dev, args.reps, res["entropy_ms"], res["h2d_bytes"])
        ent.update(image=res["image"], device=res["device"], reps=args.reps)
        ent_line = json.dumps(_rounded(ent))
        print(ent_line)
        os.makedirs(os.path.dirname(os.path.abspath(args.entropy_out)), exist_ok=True)
        with open(args.entropy_out, "w") as f:
            f.write(ent_line + "\n")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
