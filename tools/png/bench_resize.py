#!/usr/bin/env python3
"""What the resized previews cost and save: ro_stft_levels_resize_resident (csrc/ro_resize.hip) in the periodic chain, against
resizing on the host.

One step is one chunk, as in tools/png/bench_png.py: the ring is taken to hold the stream up to the chunk's end, and every
periodic snapshot that has become due in the chunk ends as a complete, RESIZED PNG file (stored blocks) in pinned host memory.
The ring's rows are real ones: the transform of Gaussian noise with a drifting tone, cut to the window's columns
(bench_png_deflate.fill_ring).
Legs, each ending with the files in pinned host memory:
  device  the plan and ro_periodic_level_dir (host arithmetic), the levels call, ro_resize_plan (host arithmetic: the taps), ONE
          upload of the blob, the out directory and its summary, the resize call, the PNG call, the files to the host (their
          sizes are host arithmetic), a wait
  twin    the plan, the levels call, the full-size levels in use to pinned host memory, a wait; then ro_resize_plan,
          ro_levels_resize_host and ro_levels_png_host over them on one host thread
  pillow  the same with Pillow's Image.resize(..., LANCZOS) of every image in the place of the twin
All are wall-clock times of the host thread.  `device call` is the time between two events around the resize call alone, 20
chunks enqueued back to back over levels and a plan already on the device (an upper bound where the host enqueues more slowly
than the device runs); `plan` is ro_resize_plan alone, sizing form and writing form, on the host.  `--repeats` alternations of
the legs, each a window of at least `--window` seconds over consecutive chunks, after one pass that checks the three legs
against each other: the same files, byte for byte.  The report goes to stdout and to `--out`.

    python tools/png/bench_resize.py [--window 0.5] [--repeats 5] [--out profiles/resize.txt]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_png_deflate import fill_ring, padded, window  # noqa: E402

BLOCK, LBLOCK, ALIGN = 2880, 720, 16
SHAPES = [  # name, sample rate, bins, overlap, snapshot_length, (low, high) Hz or None for `cols`, cols, chunk rows, width
    ("headline: 32768 bins, 75 % overlap, 615-column window, chunks of 16384 rows, --width 256", 48000, 32768, 24576, 60, None, 615,
     16384, 256),
    ("Ionozor.json VLF: 32768 bins, overlap 16384, 96 kHz, 15000 ... 30000 Hz every 300 s, chunks of 4096 rows, --width 1024", 96000,
     32768, 16384, 300, (15000.0, 30000.0), None, 4096, 1024),
]

NOTES = """\
Nothing was promised and nothing is gated on these numbers.  Reading the device-call lines: they are upper bounds of device
time.  The 20 chunks between the two events are enqueued by one Python thread; where that is slower than the device, the
figure is the enqueue rate.  Leg device pays ro_resize_plan on the host in every chunk (the `plan` line): a caller whose
shapes repeat can keep the blob on the device and pay it once.
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from PIL import Image
    ro = importlib.import_module("radio-observer_amd")
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def pinned(nbytes):
        return torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()

    say("Measured (%s, %d alternations, windows of >= %.1f s)" % (torch.cuda.get_device_name(0), args.repeats, args.window))
    say("=" * 100)
    stream = torch.cuda.current_stream().cuda_stream
    for name, rate, bins, overlap, length, band, cols, chunk, width in SHAPES:
        S = ro.snapshot_rows(rate, bins, overlap, length)
        first_col = bins // 2 + bins // 8
        if band is not None:
            first_col = ro.frequency_to_bin(bins, rate, band[0])
            cols = ro.frequency_to_bin(bins, rate, band[1]) - first_col
        recorders = [(S, 0, cols)]
        ring_rows = chunk + S + 2 + 158                  # at least S + 2 rows more than a chunk
        most = chunk // S + 2                            # snapshots a chunk can make due
        unit = padded(4 * S * cols, BLOCK)
        w2, h2 = ro.resize_shape(cols, S, width)
        out_room = most * padded(w2 * h2, LBLOCK)
        file_room = padded(ro.png_bytes(w2, h2), ALIGN)
        room, png_room = most * unit, most * file_room
        d_ring = torch.empty((ring_rows, cols), dtype=torch.float32, device="cuda")
        fill_ring(ro, torch, d_ring, bins, overlap, first_col, cols)
        with ro.Stft(bins=256, overlap=0) as st:
            ring = ro.capi.RowRing(d_ring.data_ptr(), cols, ring_rows, cols, 0)
            d_levels = torch.zeros(room // 4, dtype=torch.uint8, device="cuda")
            d_ranges = torch.zeros(most * 2, dtype=torch.float32, device="cuda")
            d_small = torch.zeros(out_room, dtype=torch.uint8, device="cuda")
            d_png = torch.zeros(png_room, dtype=torch.uint8, device="cuda")
            d_out = torch.zeros(most * 32 + 64, dtype=torch.uint8, device="cuda")    # the files' directory, then their summary
            h_png, h_levels = pinned(png_room), pinned(room // 4)
            state = {leg: [np.zeros(1, np.int64), 0] for leg in ("device", "twin", "pillow")}
            last = {}
            # the upload: the blob, then the out directory, then its summary; sized by the first plan
            probe_dir, probe_sm = ro.periodic_level_dir(ro.periodic_plan(recorders, np.zeros(1, np.int64), chunk, False, ring_rows, cols,
                                                                         room, most)[0])
            plan_room = padded(int(ro.resize_plan(probe_dir, np.array([probe_sm]), room // 4, width, out_room)[3]["plan_bytes"][0]) +
                               most * 80, ALIGN)
            d_up = torch.zeros(plan_room + most * 32 + 64, dtype=torch.uint8, device="cuda")
            h_up = pinned(plan_room + most * 32 + 64)

            def plan(leg):
                nxt, head = state[leg]
                head += chunk
                state[leg][1] = head
                return ro.periodic_plan(recorders, nxt, head, False, ring_rows, cols, room, most)

            def resize_call(info):
                st.levels_resize_resident(info, d_up, d_levels, room // 4, d_small, out_room, stream=stream)

            def leg_device():
                directory, sm = plan("device")
                st.periodic_levels_resident(ring, recorders, directory, d_ranges, d_levels, room // 4, stream=stream)
                level_dir, level_sm = ro.periodic_level_dir(directory)
                out_dir, out_sm, blob, info = ro.resize_plan(level_dir, np.array([level_sm]), room // 4, width, out_room)
                assert blob.size <= plan_room
                h = h_up.numpy()
                h[:blob.size] = blob
                h[plan_room:plan_room + len(out_dir) * 32] = out_dir.view(np.uint8)
                h[plan_room + most * 32:] = np.array([out_sm]).view(np.uint8)
                d_up.copy_(h_up, non_blocking=True)
                resize_call(info)
                st.levels_png_resident(d_up[plan_room:], most, d_up[plan_room + most * 32:], d_small, out_room, d_out, d_png, png_room,
                                       d_out[most * 32:], stream=stream)
                used = sum(padded(ro.png_bytes(int(e["naxis1"]), int(e["naxis2"])), ALIGN) for e in out_dir if e["status"] == 0)
                h_png[:used].copy_(d_png[:used], non_blocking=True)
                torch.cuda.synchronize()
                last["info"] = info
                return used

            def levels_home(leg):
                directory, sm = plan(leg)
                st.periodic_levels_resident(ring, recorders, directory, d_ranges, d_levels, room // 4, stream=stream)
                used = int(sm["units_bytes"]) // 4
                h_levels[:used].copy_(d_levels[:used], non_blocking=True)
                torch.cuda.synchronize()
                level_dir, level_sm = ro.periodic_level_dir(directory)
                return level_dir, level_sm, h_levels.numpy()[:used]

            def leg_twin():
                level_dir, level_sm, levels = levels_home("twin")
                out_dir, out_sm, blob, info = ro.resize_plan(level_dir, np.array([level_sm]), levels.size, width, out_room)
                small = ro.levels_resize_host(info, blob, levels, out_room)
                last["twin"] = ro.levels_png_host(out_dir, np.array([out_sm]), small, png_room)
                last["full"] = levels.size
                return len(last["twin"][1])

            def leg_pillow():
                level_dir, level_sm, levels = levels_home("pillow")
                out_dir = level_dir.copy()
                small = np.zeros(out_room, np.uint8)
                at = 0
                for d, e in enumerate(level_dir):
                    if e["status"] != 0:
                        continue
                    w, h = int(e["naxis1"]), int(e["naxis2"])
                    px = levels[int(e["offset"]):int(e["offset"]) + w * h].reshape(h, w)
                    ww, hh = ro.resize_shape(w, h, width)
                    if (ww, hh) != (w, h):
                        px = np.asarray(Image.fromarray(px).resize((ww, hh), Image.LANCZOS))
                    small[at:at + ww * hh] = px.reshape(-1)
                    out_dir[d] = (at, ww * hh, hh, ww, 0)
                    at += padded(ww * hh, LBLOCK)
                last["pillow"] = ro.levels_png_host(out_dir, np.array([level_sm]), small[:at], png_room)
                return len(last["pillow"][1])

            # the three legs on the first three chunks: the same files
            files = file_bytes = full_bytes = 0
            for _ in range(3):
                used = leg_device()
                got = h_png.numpy()[:used].tobytes()
                assert used > 0 and leg_twin() == used and got == last["twin"][1].tobytes(), "device and twin disagree"
                assert leg_pillow() == used and got == last["pillow"][1].tobytes(), "device and Pillow disagree"
                n = int((last["twin"][0]["status"] == 0).sum())
                files += n
                file_bytes += used
                full_bytes += n * padded(ro.png_bytes(cols, S), ALIGN)
            say("%s: S = %d, %d columns from column %d -> %d x %d; %.1f files per chunk" % (name, S, cols, first_col, w2, h2, chunk / S))
            say("  bytes downloaded: %d files, %.3f MB resized against %.3f MB full size per chunk (%.4f); leg twin downloads %.3f MB of "
                "levels" % (files, 1e-6 * file_bytes / 3, 1e-6 * full_bytes / 3, file_bytes / full_bytes, 1e-6 * last["full"]))
            legs = (("device", leg_device, "levels, plan, upload, resize, PNG call, files to the host  "),
                    ("twin", leg_twin, "levels to the host, the twin's resize and PNG writer there "),
                    ("pillow", leg_pillow, "levels to the host, Pillow's resize, the PNG writer there  "))
            t = {leg: [] for leg, _, _ in legs}
            for _ in range(args.repeats):
                for leg, fn, _ in legs:
                    t[leg].append(window(fn, args.window))
            for leg, _, what in legs:
                us = [1e6 * x for x in t[leg]]
                say("  leg %-6s %s median %10.1f us   min %10.1f   max %10.1f   %12.0f rows/s   (%s)" % (
                    leg, what, np.median(us), min(us), max(us), chunk / np.median(t[leg]), " ".join("%.1f" % x for x in us)))
            say("  time of twin over device = %.2f, of pillow over device = %.2f (medians)" % (
                np.median(t["twin"]) / np.median(t["device"]), np.median(t["pillow"]) / np.median(t["device"])))
            level_dir, level_sm = probe_dir, probe_sm
            tp = [1e6 * window(lambda: ro.resize_plan(level_dir, np.array([level_sm]), room // 4, width, out_room), args.window / 5)
                  for _ in range(args.repeats)]
            say("  plan: ro_resize_plan on the host      median %8.1f us per chunk   min %8.1f   max %8.1f" % (np.median(tp), min(tp), max(tp)))
            dev = []
            info = last["info"]
            for _ in range(args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                resize_call(info)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(20):
                    resize_call(info)
                e1.record()
                torch.cuda.synchronize()
                dev.append(1e3 * e0.elapsed_time(e1) / 20)
            say("  device call: the resize call alone   median %8.1f us per chunk   min %8.1f   max %8.1f   (%s)" % (
                np.median(dev), min(dev), max(dev), " ".join("%.1f" % x for x in dev)))
            say()
        del d_ring, d_levels, d_png, h_png, h_levels
    say(NOTES)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
