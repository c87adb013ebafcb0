#!/usr/bin/env python3
"""Benchmark of the hot path on MI355X: `python bench.py --gpus N --steps K --warmup W`.

Workload (BASELINE.json configs[1]): batch=256 random 224x224 crops through the
EfficientNet-B0 classifier, fp32, inputs resident in HBM before the timed region.  One
step = one forward over one 256-crop batch per GPU; frames shard with no data-path
collective, so N GPUs run N independent batches ("weak" scaling) and `value` is the
whole-job crops/s.  Rank 0 prints ONE JSON line.

The K timed steps are taken in turn by TWO classifier lanes per GPU (two handles of the
library = two streams and workspaces, `rtdfd_amd._lib.ClassifierLanes`): two forwards are
in flight, every forward is still one whole 256-crop batch with the same kernels and the
same result bits.  `DFD_BENCH_LANES=1` = one forward in flight (the loop of rounds 1-3).

A plain run sets up, warms up, times the K steps and prints the headline line (metric,
value, unit, ms_per_step, dtype, config) - nothing else.  `--dump-outputs DIR` writes what
the last timed step computed, its batch x 1 fp32 logits, to DIR/logits.npy (inputs and
weights are seeded: two builds compare output for output).

`--full` adds everything else.  One timed step in 20 then carries the per-launch HIP events
and is ordered ALONE on the device (`dfd_wait_for`), so the roofline durations are those of
isolated kernels; the overlap that step gives up is inside the timed region.  After the
timed loop: lane-equality and oracle-parity checks, and the extra objects below
(`--no-e2e`, `--no-streams`, `--no-cpu-baseline` leave single ones out).

Extra objects on a --full line:
  roofline      depthwise-conv kernel family against the HBM roofline: algorithmic bytes
                (25.11 MB per crop) x crops per launch-set / the 16 depthwise
                launches' duration, measured with HIP events on the library's stream
                inside the timed region
  cpu_baseline  the CPU oracle (torch-CPU fp32 restatement of the reference path) timed
                on this host's cores on a bounded sample, rank 0 at N=1 only
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0     # /opt/skills/guides/MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
BATCH = 256
LANES = max(1, int(os.environ.get("DFD_BENCH_LANES", "2")))     # classifier forwards in flight in the headline loop
PROFILE_EVERY = 20        # every 20th timed step carries the per-launch events and runs alone (~0.7 ms of lost overlap each)
E2E_FRAMES = 64


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(sd_np, with_e2e=True):
    """Times the CPU oracle (the checker; used here only as the CPU baseline) on a bounded sample of the same
    workloads, SURVEY 8(d) "CPU baseline beside it": the classifier at reference-style batch 1 and at batch 256,
    and - beside the e2e object - detector, CLAHE + 224 resize, and the six forensic signals per 1080p frame."""
    import torch

    import rtdfd_amd
    from oracle import b0_ref

    # the cores this process may actually use (the GPU box gives a 1-GPU job a 16-core share;
    # os.cpu_count() there reports the whole host and oversubscribes torch's pool 16x)
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, int(os.environ.get("DFD_CPU_THREADS", "16"))))
    torch.set_num_threads(cores)
    sd = rtdfd_amd.weights.to_torch(sd_np)
    torch.manual_seed(1)
    x = torch.randn(BATCH, 3, 224, 224)
    b0_ref.forward(sd, x[:2])                       # warm-up

    def samples(fn, n):
        out = []
        for _ in range(n):
            t = time.perf_counter()
            fn()
            out.append(time.perf_counter() - t)
        return out

    # three modes, several samples each (a single 8.7 s forward was round 2's whole measurement):
    #   batch 1   - the STATED baseline (`value`): how the reference drives the classifier, one crop per request
    #               (backend_server.py:160-164 -> deepfake_detection.py:391-398), 24 calls;
    #   batch 16  - cache-friendlier chunks, 4 calls;
    #   batch 256 - the benchmark's own step on the CPU, 2 calls (8-9 s each on 16 cores: the bound on this leg).
    s1 = samples(lambda: b0_ref.forward(sd, x[:1]), 24)
    s16 = samples(lambda: b0_ref.forward(sd, x[:16]), 4)
    s256 = samples(lambda: b0_ref.forward(sd, x), 2)
    med = lambda v: sorted(v)[len(v) // 2]                               # noqa: E731
    dt1, dt16, dt256 = med(s1), med(s16) / 16, min(s256)
    out = {"value": round(1.0 / dt1, 2), "unit": "crops/s", "cores": torch.get_num_threads(), "kind": "port",
           "cpu_model": cpu_model(), "stated_mode": "batch 1 (reference-style: one crop per /analyze request)",
           "sample": f"torch-CPU fp32 oracle: 24 batch-1 forwards (median {dt1 * 1e3:.1f} ms, min {min(s1) * 1e3:.1f}, max "
                     f"{max(s1) * 1e3:.1f}); 4 batch-16 forwards (median {med(s16) * 1e3:.0f} ms); 2 batch-{BATCH} forwards "
                     f"({s256[0]:.2f} s, {s256[1]:.2f} s)",
           "batch1_crops_per_s": round(1.0 / dt1, 2), "batch16_crops_per_s": round(1.0 / dt16, 2),
           "batch256_crops_per_s": round(BATCH / dt256, 2),
           "samples_ms": {"batch1": [round(v * 1e3, 2) for v in s1], "batch16": [round(v * 1e3, 1) for v in s16],
                          "batch256": [round(v * 1e3, 0) for v in s256]}}
    if with_e2e:
        from oracle import forensics_ref, imgproc_ref, ssd_ref

        W = rtdfd_amd.weights
        ssd_sd = W.to_torch(W.seeded_ssd_state_dict(0))
        frame = np.random.default_rng(7).integers(50, 200, (1080, 1920, 3), dtype=np.uint8)
        boxes = [(200, 150, 320, 400), (900, 300, 256, 256), (1400, 500, 400, 480), (600, 700, 224, 224)]

        def timed(fn, reps):
            fn()
            t = time.perf_counter()
            for _ in range(reps):
                fn()
            return (time.perf_counter() - t) / reps

        t_det = timed(lambda: ssd_ref.detect_bounding_box(ssd_sd, rtdfd_amd.ssd_arch, frame), 3)
        t_pre = timed(lambda: [imgproc_ref.crop_resize_normalize(imgproc_ref.preprocess_face_quality(
            frame[y:y + h, x0:x0 + w])) for (x0, y, w, h) in boxes], 2)
        an = forensics_ref.ForensicsRef()
        t_for = timed(lambda: an.analyze(frame), 2)
        t_cls = dt1 * len(boxes)
        per_frame = t_det + t_pre + t_cls
        out["e2e_port"] = {
            "workload": "one 1080p frame, 4 forced boxes: detector (300x300 SSD) + CLAHE/224 resize + B0 batch 1 per face",
            "detect_ms": round(t_det * 1e3, 1), "clahe_resize_ms_4_faces": round(t_pre * 1e3, 1),
            "classify_ms_4_faces": round(t_cls * 1e3, 1), "forensics_full_ms": round(t_for * 1e3, 1),
            "detect_classify_frames_per_s": round(1.0 / per_frame, 2),
            "detect_classify_forensics_frames_per_s": round(1.0 / (per_frame + t_for), 2)}
    return out


# DFD_BENCH_REHEARSE=1: the --gpus N code path of this file on a box with fewer GPUs than ranks (ranks share devices,
# torch.distributed over gloo with CPU tensors, vote exchange on the documented torch fallback) - a rehearsal of the
# multi-rank control flow on real hardware, never a measurement
REHEARSE = os.environ.get("DFD_BENCH_REHEARSE") == "1"


def _red_dev(local_rank):
    return "cpu" if REHEARSE else f"cuda:{local_rank}"


def e2e_frames(h, rank, dist, local_rank, frames_per_step=E2E_FRAMES, steps=6, warmup=3, blob=None):
    """BASELINE.json configs[2]/[3] as an extra: 1080p synthetic frames resident in HBM ->
    SSD detect (every frame) + 4 forced >=224x224 boxes per frame -> CLAHE -> 224x224 -> B0, without and
    with the six forensic signals.  Frames: np.random.default_rng(7 + rank).integers(50, 200)."""
    import torch

    H, W, K = 1080, 1920, 4
    rng = np.random.default_rng(7 + rank)
    frames = rng.integers(50, 200, (frames_per_step, H, W, 3), dtype=np.uint8)
    fd = h.alloc(frames.nbytes).upload(frames)
    boxes = [[(200, 150, 320, 400), (900, 300, 256, 256), (1400, 500, 400, 480), (600, 700, 224, 224)]] * frames_per_step
    res = {"workload": f"{frames_per_step} x 1080p frames/step, SSD detect + {K} forced boxes/frame -> CLAHE -> 224 -> B0 fp32",
           "frames_per_step": frames_per_step}
    def run(forensic, k):
        h.sync()
        if dist is not None:
            dist.barrier()
        t0 = time.perf_counter()
        for _ in range(k):
            h.analyze_batch_device(fd.ptr, frames_per_step, H, W, forced_boxes=boxes, max_faces=K, with_forensics=forensic)
        h.sync()
        dt = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([dt], dtype=torch.float64, device=_red_dev(local_rank))
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    # untimed: lazy workspace growth, clock ramp-up and whatever one-off cost follows the classifier run
    # (the first timed loop after it was reproducibly ~2x slow, whichever configuration came first)
    for forensic in (False, True, False, True):
        run(forensic, warmup)
    world = 1 if dist is None else dist.get_world_size()
    for key, forensic, bf16 in (("detect_classify", False, 0), ("detect_classify_forensics", True, 0),
                                ("detect_classify_forensics_bf16", True, 1)):
        h.set_option("bf16_activations", bf16)
        if bf16:
            h.warmup(h.max_batch, 0)                         # the bf16 GEMM instances have their own tile table entries
            run(forensic, warmup)
        dts = sorted(run(forensic, steps) for _ in range(3))
        dt = dts[1]                                          # median of three timed repeats
        res[key] = {"frames_per_s": round(frames_per_step * steps * world / dt, 1),
                    "crops_per_s": round(frames_per_step * K * steps * world / dt, 1),
                    "ms_per_frame": round(dt / (frames_per_step * steps) * 1e3, 3),
                    "repeats_frames_per_s": [round(frames_per_step * steps * world / d, 1) for d in dts]}
    h.set_option("bf16_activations", 0)
    # the same call with TWO of them in flight: a second handle (its own streams and workspaces, the same tile table) driven
    # by a second host thread (the library calls release the GIL) - a server with two workers on one GPU.  One call is a
    # chain of ~150 dependent launches and three stream waits; the other call's kernels fill its gaps and under-filled tails.
    h2 = None

    def second_handle():
        # its main stream at HIGH priority: streams of one priority share a small pool of hardware queues, and in this
        # process (seven streams made before this one) a second normal-priority main stream ended up in line with h's -
        # 12.6 k frames/s with two calls in flight instead of 14.4 k (profiles/e2e_lanes_probe.py, PROBE_PRELUDE=ABCD).
        # Created for these rows only and closed after them: the single-call rows run in a process without it.
        import rtdfd_amd

        hh = rtdfd_amd._lib.Handle(blob, device=local_rank, max_batch=h.max_batch)
        hh.set_option("stream_priority", 1)
        hh.tiles_import(h.tiles_export())
        hh.warmup(h.max_batch, frames_per_step)
        return hh

    # JPEG BYTES across PCIe instead of raw frames (reference backend_server.py:139-145 receives JPEG):
    # dfd_analyze_jpegs_host - the scans of chunk k + 1 are uploaded while chunk k is entropy-decoded ON THE DEVICE
    # (csrc/jpeg_gpu_entropy.h), turned into frames and analysed.  Two kinds of quality-85 4:2:0 frames, byte sizes stated:
    # a natural-texture frame (smooth shading + texture + sensor noise) and the random-texture frames of the rows above
    # (the worst case for entropy coding: 4 x the bytes of a natural frame).
    if world == 1:
        import io

        from PIL import Image

        def encode(fr):
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(fr[..., ::-1])).save(buf, format="JPEG", quality=85)
            return buf.getvalue()

        def natural_texture(seed):
            r = np.random.default_rng(seed)
            yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
            img = np.zeros((H, W, 3), np.float32)
            for c in range(3):
                img[..., c] = 120 + 60 * np.sin(xx / (190.0 + 23 * c) + c) * np.cos(yy / (140.0 - 11 * c)) + 25 * np.sin((xx + 2 * yy) / 37.0)
            low = r.normal(0, 1, (H // 8 + 1, W // 8 + 1, 3)).astype(np.float32)
            img += 14 * np.kron(low, np.ones((8, 8, 1), np.float32))[:H, :W]      # blocky mid-frequency texture
            img += r.normal(0, 3.0, img.shape)                                    # sensor noise
            return np.clip(img, 0, 255).astype(np.uint8)

        reps = 8
        rows = {}
        deferred_jpeg = []
        for kind, src in (("natural_texture", [natural_texture(40 + i) for i in range(8)]), ("random_texture", [frames[i] for i in range(8)])):
            files = [encode(f) for f in src]
            datas = [files[i % len(files)] for i in range(reps * frames_per_step)]
            packed = h.pack_jpegs(datas)
            hb = boxes * reps
            best = None
            for chunk in (64, 32):
                for _ in range(3):                                  # untimed: buffers, clocks (the files were just encoded on the host)
                    h.analyze_jpegs_host(datas, chunk, forced_boxes=hb, max_faces=K, packed=packed)
                dts = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    h.analyze_jpegs_host(datas, chunk, forced_boxes=hb, max_faces=K, packed=packed)
                    dts.append(time.perf_counter() - t0)
                dt = sorted(dts)[2]
                if best is None or dt < best[1]:
                    best = (chunk, dt)
            on_dev, on_host = h.jpeg_decode_counts()
            rows[kind] = {"frames_per_s": round(len(datas) / best[1], 1), "ms_per_frame": round(best[1] / len(datas) * 1e3, 3),
                          "frames_per_chunk": best[0], "jpeg_bytes_per_frame": int(np.mean([len(f) for f in files])),
                          "MB_per_s_over_pcie": round(sum(len(d) for d in datas) / best[1] / 1e6, 1)}
            h.host_free(packed[0])
            deferred_jpeg.append((kind, datas, hb, best[0]))
        rows["frames_entropy_decoded_on_device_vs_host_decoder"] = list(h.jpeg_decode_counts())
        rows["note"] = (f"{reps * frames_per_step} x 1080p quality-85 4:2:0 JPEG files from pinned host memory per call, SSD detect + {K} "
                        "forced boxes -> CLAHE -> 224 -> B0 fp32 as the rows above; decoded frames equal Pillow's bit for bit "
                        "(tests/test_jpeg_decode.py); the raw-frame path of the row above is bound by its 6.2 MB per frame")
        res["detect_classify_jpeg_h2d"] = rows
    # PCIe-inclusive: the same frames from pinned host memory, 8 x 64 frames per call in batches of 64, the upload
    # of batch k + 1 overlapped with the compute of batch k (dfd_analyze_frames_host)
    if world == 1:
        reps = 8
        pinned = h.host_alloc((reps * frames_per_step, H, W, 3))
        for r in range(reps):
            pinned[r * frames_per_step:(r + 1) * frames_per_step] = frames
        hboxes = boxes * reps
        # chunk size: measured, not assumed
        h.warmup(min(32 * K, h.max_batch), 32)
        h.warmup(min(16 * K, h.max_batch), 16)
        by_chunk = {}
        for chunk in (64, 32, 16):
            h.analyze_frames_host(pinned, chunk, forced_boxes=hboxes, max_faces=K)
            dts = []
            for _ in range(3):
                t0 = time.perf_counter()
                h.analyze_frames_host(pinned, chunk, forced_boxes=hboxes, max_faces=K)
                dts.append(time.perf_counter() - t0)
            by_chunk[chunk] = sorted(dts)[1]
        best_chunk = min(by_chunk, key=by_chunk.get)
        dt = by_chunk[best_chunk]
        tmp = h.alloc(pinned.nbytes // reps)
        h.sync()
        t0 = time.perf_counter()
        for r in range(reps):
            tmp.upload(pinned[r * frames_per_step:(r + 1) * frames_per_step])
        h2d = time.perf_counter() - t0
        tmp.free()
        nfr = reps * frames_per_step
        res["detect_classify_h2d"] = {
            "frames_per_s": round(nfr / dt, 1), "ms_per_frame": round(dt / nfr * 1e3, 3),
            "upload_only_frames_per_s": round(nfr / h2d, 1), "upload_GBps": round(pinned.nbytes / h2d / 1e9, 1),
            "bound": "PCIe upload" if nfr / h2d < res["detect_classify"]["frames_per_s"] else "GPU compute",
            "frames_per_chunk": best_chunk,
            "frames_per_s_by_chunk": {str(c): round(nfr / t, 1) for c, t in by_chunk.items()},
            "note": f"{nfr} x 1080p frames from pinned host memory per call, in chunks (the best of 64 / 32 / 16 frames is the "
                    "stated row), upload of chunk k+1 on a second "
                    "stream during chunk k (the first upload of a call is not overlapped); descriptors / detections / logits "
                    "move through a pinned mailbox with copy kernels so that they do not queue behind the frame upload on the "
                    "SDMA engine; 6.22 MB per frame over PCIe Gen5 x16 (63 GB/s spec)"}
        h.host_free(pinned)
        if "detect_classify_jpeg_h2d" in res:
            res["detect_classify_jpeg_h2d"]["raw_upload_bound_frames_per_s"] = res["detect_classify_h2d"]["upload_only_frames_per_s"]
        # the same with a four times longer call: the un-overlapped ends of a call (first upload, last chunk's compute) are
        # a fixed cost, so the rate of a long call is the one a continuously fed service sees
        long_reps = 4 * reps
        try:
            pinned = h.host_alloc((long_reps * frames_per_step, H, W, 3))
        except Exception:                                   # not enough pinned host memory on this box: skip the row
            pinned = None
        if pinned is not None:
            for r in range(long_reps):
                pinned[r * frames_per_step:(r + 1) * frames_per_step] = frames
            lboxes = boxes * long_reps
            h.analyze_frames_host(pinned, best_chunk, forced_boxes=lboxes, max_faces=K)
            dts = []
            for _ in range(2):
                t0 = time.perf_counter()
                h.analyze_frames_host(pinned, best_chunk, forced_boxes=lboxes, max_faces=K)
                dts.append(time.perf_counter() - t0)
            res["detect_classify_h2d"]["long_call"] = {"frames": long_reps * frames_per_step,
                                                       "frames_per_s": round(long_reps * frames_per_step / min(dts), 1),
                                                       "frames_per_chunk": best_chunk}
            h.host_free(pinned)
    # per-request latency of the server flow from JPEG bytes: entropy decode on the host + IDCT / colour on
    # the device (dfd_analyze_jpeg) against host decode (Pillow) + raw upload (dfd_analyze_frame)
    if world == 1:
        import io

        from PIL import Image

        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(frames[0][..., ::-1])).save(buf, format="JPEG", quality=85)
        data = buf.getvalue()

        def t_ms(fn, reps=8):
            fn()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            return (time.perf_counter() - t0) / reps * 1e3

        def host_path():
            fr = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])
            h.analyze_frame(fr, True, stream_id=990, max_faces=1)

        res["request_1080p_jpeg"] = {"jpeg_bytes": len(data),
                                     "device_decode_ms": round(t_ms(lambda: h.analyze_jpeg(data, True, stream_id=991, max_faces=1)), 2),
                                     "host_decode_ms": round(t_ms(host_path), 2),
                                     "note": "one /analyze request body: forensics (full) + detect + faces[0] classify; quality-85 4:2:0 "
                                             "JPEG of a random-texture 1080p frame (worst case for entropy coding)"}
    res["detect_classify_forensics_bf16"]["arithmetic"] = (
        "configs[3]: classifier activations stored as bf16 (fp32 accumulate, fp32-exact weights); detector, CLAHE and "
        "forensic kernels unchanged (integer / fp32: box indices must stay bit-exact); vote-equality gate: "
        "tests/test_b0_bf16_gpu.py::test_config4_gate_votes_equal_fp32_oracle_on_200_frames")
    if rank == 0 and world == 1:
        res["detect_classify_mtcnn"] = e2e_mtcnn(frames, boxes, K)
    # ---- the rows with TWO calls in flight, after every single-call row (their extra handle, its streams and their
    # hardware queues must not be part of the process the single-call rows are measured in)
    if world == 1 and blob is not None:
        try:
            import threading

            h2 = second_handle()
            if True:
                def calls(hh, forensic, k, keep):
                    r = None
                    for _ in range(k):
                        r = hh.analyze_batch_device(fd.ptr, frames_per_step, H, W, forced_boxes=boxes, max_faces=K, with_forensics=forensic)
                    keep.append(r)

                for key, forensic in (("detect_classify_two_calls_in_flight", False), ("detect_classify_forensics_two_calls_in_flight", True)):
                    want = []
                    calls(h, forensic, 1, want)
                    calls(h2, forensic, warmup, [])
                    dts, same = [], True
                    for _ in range(3):
                        got = [[], []]
                        th = [threading.Thread(target=calls, args=(hh, forensic, steps, got[i])) for i, hh in enumerate((h, h2))]
                        h.sync(); h2.sync()
                        t0 = time.perf_counter()
                        for t in th:
                            t.start()
                        for t in th:
                            t.join()
                        dts.append(time.perf_counter() - t0)
                        for g in got:
                            same = same and g[0][0] == want[0][0] and np.array_equal(
                                np.asarray(g[0][1], np.float32), np.asarray(want[0][1], np.float32), equal_nan=True)
                    dts.sort()
                    res[key] = {"frames_per_s": round(frames_per_step * steps * 2 / dts[1], 1), "calls_in_flight": 2,
                                "repeats_frames_per_s": [round(frames_per_step * steps * 2 / d, 1) for d in dts],
                                "boxes_and_logits_equal_the_single_call": bool(same)}
            for kind, datas, hb, chunk in (deferred_jpeg if "detect_classify_jpeg_h2d" in res else []):
                # the same files as TWO calls in flight (two handles, two host threads, half of the files each): one call's
                # decode passes are latency-bound chains; the other call's kernels run beside them
                half = len(datas) // 2
                parts = [(hh, datas[k * half:(k + 1) * half], hb[k * half:(k + 1) * half]) for k, hh in enumerate((h, h2))]
                packs = [hh.pack_jpegs(d) for hh, d, _ in parts]

                def jcall(k, keep):
                    hh, d, b = parts[k]
                    keep.append(hh.analyze_jpegs_host(d, chunk, forced_boxes=b, max_faces=K, packed=packs[k]))

                def both():
                    keep = [[], []]
                    th = [threading.Thread(target=jcall, args=(k, keep[k])) for k in range(2)]
                    t0 = time.perf_counter()
                    for t in th:
                        t.start()
                    for t in th:
                        t.join()
                    return time.perf_counter() - t0, keep

                for _ in range(3):
                    both()
                dts = sorted(both()[0] for _ in range(5))
                res["detect_classify_jpeg_h2d"][kind]["two_calls_in_flight_frames_per_s"] = round(2 * half / dts[2], 1)
                for k, (hh, _, _) in enumerate(parts):
                    hh.host_free(packs[k][0])
            h2.close()
            h2 = None
        except Exception as e:                                   # noqa: BLE001 - an extra row must never cost the line
            res["two_calls_in_flight_error"] = f"{type(e).__name__}: {e}"
            if h2 is not None:
                try:
                    h2.close()
                except Exception:                                # noqa: BLE001
                    pass
    fd.free()
    return res


def e2e_mtcnn(frames, boxes, K):
    """The same path with the reference's MTCNN align/crop between CLAHE and the 224x224 resize (row A5), on a
    handle whose blob carries the (seeded) cascade: all crops of a call go through the three stages together, box
    bookkeeping between the stages on the library's host side."""
    import rtdfd_amd as pkg

    W = pkg.weights
    H, Wd = frames.shape[1:3]
    out = {}
    handles = {}
    blobs = {}
    # (key, option "mtcnn", head-bias recipe, frames per call): the 8-frame rows are per-call latency figures (every stage
    # of a call runs at a small batch), the 64-frame rows the batched throughput of the same path
    # "..._forensics": every stage of the reference's per-frame flow on (detect, CLAHE, MTCNN, classify, six signals)
    for key, flag, bias, n in (("mtcnn_on", 1, None, 8), ("mtcnn_off", 0, None, 8), ("mtcnn_on_selective", 1, W.MTCNN_SELECTIVE, 8),
                               ("mtcnn_on_selective_64", 1, W.MTCNN_SELECTIVE, len(frames)),
                               ("mtcnn_on_selective_64_forensics", 1, W.MTCNN_SELECTIVE, len(frames)),
                               ("mtcnn_off_64", 0, W.MTCNN_SELECTIVE, len(frames))):
        tag = "sel" if bias else "dense"
        if tag not in handles:
            blobs[tag] = W.pack_all(W.seeded_state_dict(0), W.seeded_ssd_state_dict(0), W.seeded_mtcnn_state_dict(0, bias))
            hh = pkg._lib.Handle(blobs[tag], device=0, max_batch=len(frames) * K)
            hh.warmup(len(frames) * K, len(frames))             # classifier / detector GEMM tiles, as for the main handle
            hh.warmup(8 * K, 8)
            handles[tag] = (hh, hh.alloc(frames.nbytes).upload(frames))
        h, fd = handles[tag]
        h.set_option("mtcnn", flag)
        bx = boxes[:n]
        wf = key.endswith("_forensics")
        for _ in range(2):
            h.analyze_batch_device(fd.ptr, n, H, Wd, forced_boxes=bx, max_faces=K, with_forensics=wf)
        h.sync()
        # every call returns its results (it ends with a stream wait): per-call wall times, the median is the stated rate
        # (a process-level one-off - e.g. the interpreter's first full collection, ~40 ms - must not decide a 7 ms figure)
        calls = []
        for _ in range(3 if key == "mtcnn_on" else 9):
            t0 = time.perf_counter()
            res = h.analyze_batch_device(fd.ptr, n, H, Wd, forced_boxes=bx, max_faces=K, with_forensics=wf)
            calls.append(time.perf_counter() - t0)
        dt = sorted(calls)[len(calls) // 2]
        flat = np.concatenate([np.asarray(l, np.float32).reshape(-1) for l in res[1]]) if len(res[1]) else np.zeros(0)
        out[key] = {"frames_per_s": round(n / dt, 1), "ms_per_crop": round(dt / (n * K) * 1e3, 3),
                    "ms_per_call_min_median_max": [round(min(calls) * 1e3, 2), round(dt * 1e3, 2), round(max(calls) * 1e3, 2)],
                    "crops_with_a_face": int((~np.isnan(flat)).sum()), "crops": int(flat.size), "frames_per_call": n}
    # every stage of the reference flow on, TWO calls in flight (second handle on a high-priority main stream, second host
    # thread), after the single-call rows of this section
    import threading

    h, fd = handles["sel"]
    h.set_option("mtcnn", 1)
    h2 = pkg._lib.Handle(blobs["sel"], device=0, max_batch=len(frames) * K)
    try:
        h2.set_option("stream_priority", 1)
        h2.tiles_import(h.tiles_export())
        h2.warmup(len(frames) * K, len(frames))
        n = len(frames)

        def worker(hh, k, keep):
            r = None
            for _ in range(k):
                r = hh.analyze_batch_device(fd.ptr, n, H, Wd, forced_boxes=boxes[:n], max_faces=K, with_forensics=True)
            keep.append(r)

        want = []
        worker(h, 1, want)
        worker(h2, 2, [])
        dts, same = [], True
        for _ in range(3):
            got = [[], []]
            th = [threading.Thread(target=worker, args=(hh, 5, got[i])) for i, hh in enumerate((h, h2))]
            t0 = time.perf_counter()
            for t in th:
                t.start()
            for t in th:
                t.join()
            dts.append(time.perf_counter() - t0)
            for g in got:
                same = same and g[0][0] == want[0][0] and all(
                    np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32), equal_nan=True) for a, b in zip(g[0][1], want[0][1]))
        dts.sort()
        out["mtcnn_on_selective_64_forensics_two_calls_in_flight"] = {
            "frames_per_s": round(n * 10 / dts[1], 1), "calls_in_flight": 2, "frames_per_call": n,
            "repeats_frames_per_s": [round(n * 10 / d, 1) for d in dts], "boxes_and_logits_equal_the_single_call": bool(same)}
    except Exception as e:                                       # noqa: BLE001 - an extra row must never cost the line
        out["mtcnn_on_selective_64_forensics_two_calls_in_flight"] = {"error": f"{type(e).__name__}: {e}"}
    finally:
        h2.close()
    n = 8
    out["workload"] = (f"1080p frames, {K} forced boxes each, frames_per_call as listed; seeded random-init cascade: 'mtcnn_on' = "
                       "stress cascade (~20 % of the P-Net cells and ~99 % of the R-Net candidates pass: hundreds of windows per "
                       "crop reach O-Net), 'mtcnn_on_selective*' = the funnel of a trained cascade (weights.MTCNN_SELECTIVE)")
    for h, fd in handles.values():
        fd.free()
        h.close()
    return out


def vote_gate(logits_fp32, logits_bf16, frames=200):
    """What bf16 storage does to the VOTE (SURVEY 8(d) Config 4 gate), at thresholds nobody picked for it: the first
    `frames` crops of the batch as a stream of face probabilities, voted with the reference's tracker (10-vote window) at
    the reference's thresholds 0.5 / 0.55 (deepfake_detection.py:730, backend_server.py:57) and at 32 thresholds on the
    quantiles of the fp32 probabilities.  Per threshold: votes that differ between the fp32 and the bf16 run, frames whose
    majority verdict differs, and the fp32 probabilities within the largest bf16 error of the threshold (the only
    frames a bf16-sized error can flip).  The 200-frame gate against the fp32 ORACLE through detector + CLAHE is
    tests/test_b0_bf16_gpu.py::test_config4_gate_*."""
    from rtdfd_amd.tracker import TemporalTracker

    sig = lambda v: 1.0 / (1.0 + np.exp(-np.asarray(v, np.float32).ravel()[:frames].astype(np.float32)))     # noqa: E731
    p32, p16 = sig(logits_fp32), sig(logits_bf16)
    err = float(np.abs(p32 - p16).max())
    thresholds = [0.5, 0.55] + [float(q) for q in np.quantile(p32, np.linspace(0.03, 0.97, 32))]

    def verdicts(p, thr):
        tr = TemporalTracker(voting_window=10, detection_threshold=thr)
        out = []
        for v in p:
            tr.update(float(v))
            out.append(tr.get_confidence_level())
        return out

    rows = []
    for thr in thresholds:
        fv = int(np.sum((p32 > thr) != (p16 > thr)))
        fd = sum(1 for a, b in zip(verdicts(p32, thr), verdicts(p16, thr)) if a != b)
        rows.append({"threshold": round(thr, 5), "flipped_votes": fv, "flipped_verdict_frames": fd,
                     "frames_within_bf16_error": int(np.sum(np.abs(p32 - thr) <= err))})
    return {"frames": int(p32.size), "max_abs_prob_err": err,
            "flipped_votes_total": int(sum(r["flipped_votes"] for r in rows)), "votes_total": int(p32.size * len(rows)),
            "flipped_verdict_frames_total": int(sum(r["flipped_verdict_frames"] for r in rows)),
            "thresholds_with_a_flip": int(sum(1 for r in rows if r["flipped_votes"])), "per_threshold": rows}


def bf16_classify(h, xd, yd, batch, steps, logits_fp32, dw_bytes_bf16):
    """configs[3]'s classifier half as its own object: the batch-256 step with bf16 activation storage, its own
    depthwise roofline on 12.55 MB per crop, and the logit error against the fp32 run of the same crops."""
    out = {}
    for key, planes in (("weights_fp32_exact", 3), ("weights_bf16", 1)):
        h.set_option("bf16_activations", 1)
        h.set_option("bf16_weight_planes", planes)
        h.warmup(batch, 0)
        for _ in range(3):
            h.classify_device(xd.ptr, batch, yd.ptr)
        h.sync()
        h.set_option("profile_stride", 4)
        h.profile_begin()
        t0 = time.perf_counter()
        for _ in range(steps):
            h.classify_device(xd.ptr, batch, yd.ptr)
        h.sync()
        dt = time.perf_counter() - t0
        seen, layers = h.profile_end()
        y = yd.download((batch, 1))
        dw_ms = sum(ms for name, ms in layers if name.endswith(".dw")) / max(seen, 1)
        ach = dw_bytes_bf16 / (dw_ms * 1e-3) / 1e9 if dw_ms > 0 else 0.0
        out[key] = {"crops_per_s": round(batch * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3),
                    "max_abs_logit_err_vs_fp32_run": float(np.abs(y - logits_fp32).max()),
                    "roofline": {"bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                 "frac": round(ach / HBM_PEAK_GBS, 4), "algorithmic_bytes_per_step": dw_bytes_bf16,
                                 "ms_per_step": round(dw_ms, 4)},
                    "ms_by_kind": {k: round(sum(ms for n_, ms in layers if n_.split(".")[-1] == k) / max(seen, 1), 3)
                                   for k in ("dw", "se", "proj", "exp", "head", "avgpool", "mlp")},
                    "vote_gate": vote_gate(logits_fp32, y)}
    h.set_option("bf16_activations", 0)
    h.set_option("bf16_weight_planes", 3)
    out["dtype"] = "bf16 activation storage, f32 accumulate (depthwise bytes 12.55 MB per crop)"
    return out


def bf16_two_lanes(lanes, xd, ys, batch, steps):
    """configs[3]'s classifier half with TWO forwards in flight (the headline loop with bf16 activation storage), before
    the second lane is closed: {weights variant: crops/s}.  The per-launch numbers of the bf16 rows come from the
    one-forward loop of `bf16_classify`."""
    out = {}
    try:
        for key, planes in (("weights_fp32_exact", 3), ("weights_bf16", 1)):
            lanes.set_option("bf16_activations", 1)
            lanes.set_option("bf16_weight_planes", planes)
            lanes.warmup(batch)
            lanes._next = 0
            for i in range(4):
                lanes.submit(xd.ptr, batch, ys[i % len(lanes)].ptr)
            lanes.sync()
            t0 = time.perf_counter()
            for i in range(steps):
                lanes.submit(xd.ptr, batch, ys[i % len(lanes)].ptr)
            lanes.sync()
            dt = time.perf_counter() - t0
            same = all(np.array_equal(ys[k].download((batch, 1)), ys[0].download((batch, 1))) for k in range(1, len(lanes)))
            out[key] = {"crops_per_s": round(batch * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3),
                        "forwards_in_flight": len(lanes), "lanes_agree_bitwise": bool(same)}
    finally:
        lanes.set_option("bf16_activations", 0)
        lanes.set_option("bf16_weight_planes", 3)
    return out


def separate_late_launches(h, xd, yd, batch, steps, logits_fp32):
    """The same fp32 step with option "fuse_late" OFF (round 3's headline configuration): blocks 6-15 as expand GEMM +
    depthwise kernel, the expanded tensor through memory.  Slower per step; its 16 depthwise launches hold no expand work
    for blocks 6-15, so the SURVEY 8(d) fraction of those launches is higher - reported beside the headline so that both
    numbers stay comparable across rounds."""
    h.set_option("fuse_late", 0)
    try:
        h.warmup(batch, 0)
        for _ in range(3):
            h.classify_device(xd.ptr, batch, yd.ptr)
        h.sync()
        h.set_option("profile_stride", 4)
        h.profile_begin()
        t0 = time.perf_counter()
        for _ in range(steps):
            h.classify_device(xd.ptr, batch, yd.ptr)
        h.sync()
        dt = time.perf_counter() - t0
        seen, layers = h.profile_end()
        y = yd.download((batch, 1))
    finally:
        h.set_option("fuse_late", 1)
    dw_ms = sum(ms for name, ms in layers if name.endswith(".dw")) / max(seen, 1)
    return {"crops_per_s": round(batch * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3),
            "dw_family_ms_per_step": round(dw_ms, 4),
            "ms_by_kind": {k: round(sum(ms for n_, ms in layers if n_.split(".")[-1] == k) / max(seen, 1), 3)
                           for k in ("dw", "se", "proj", "exp", "head", "avgpool", "mlp")},
            "max_abs_logit_diff_vs_headline_run": float(np.abs(y - logits_fp32).max())}


def one_forward_in_flight(h, xd, yd, batch, steps, logits_fp32):
    """The same batch-256 forwards with ONE of them in flight (the headline loop of rounds 1-3): what a caller that
    waits for each batch before queueing the next gets from the same kernels."""
    for _ in range(2):
        h.classify_device(xd.ptr, batch, yd.ptr)
    h.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        h.classify_device(xd.ptr, batch, yd.ptr)
    h.sync()
    dt = time.perf_counter() - t0
    y = yd.download((batch, 1))
    return {"crops_per_s": round(batch * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps,
            "forwards_in_flight": 1, "max_abs_logit_diff_vs_headline_run": float(np.abs(y - logits_fp32).max())}


def stream_frame(base, t):
    """frame t of a synthetic 1080p stream: the stream's base frame with a band that scrolls 4 px per frame and a
    patch whose brightness follows t - cheap to make, deterministic in (base, t), frame-to-frame mean |diff| ~ 1"""
    f = base.copy()
    y0 = (37 * t) % (base.shape[0] - 256)
    f[y0:y0 + 256] = np.roll(base[y0:y0 + 256], 4 * (t + 1), axis=1)
    f[64:192, 64:192] = np.clip(base[64:192, 64:192].astype(np.int16) + ((t * 7) % 23) - 11, 0, 255).astype(np.uint8)
    return f


def config5_streams(h, rank, world, dist, local_rank, waves=32, n_streams=8, verify_frames=None, lookahead=8,
                    size=(1080, 1920), extra_handles=()):
    """BASELINE.json configs[4] / SURVEY 8(d) Config 5: 8 seeded 1080p streams (seeds 100-107), frame t of every
    stream on rank t % G (weak scaling: 8 frames per GPU per wave), per wave ONE all-gather of 80-byte records
    (dfd_vote_allgather = ncclAllGather over RCCL through the C ABI; torch.distributed as a fallback) inside the
    timed loop, then every rank replays temporal forensic signal + votes in frame order.  After the timed loop rank 0
    recomputes the single-GPU sequence of ALL frames and requires identical verdict sequences.  `h` only needs the
    handle methods used here (tests/test_streams.py drives this function at world 2 over gloo with a CPU stand-in, so
    the --gpus N branch has run somewhere before the driver's first multi-GPU launch)."""
    import torch

    from rtdfd_amd import streams as S

    Hh, Ww = size
    on_gpu = torch.cuda.is_available()

    def fence():                                                 # barrier + device sync on both sides of the timed region
        h.sync()
        if dist is not None:
            dist.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    bases = [np.random.default_rng(100 + s).integers(50, 200, (Hh, Ww, 3), dtype=np.uint8) for s in range(n_streams)]
    # RCCL through the C ABI, or - decided by ALL ranks together - the documented torch.distributed fallback: rank 0's
    # id (or its failure) is broadcast either way, and the ranks agree on the outcome of comm_init with a MIN all-reduce
    # (a rank that fell back on its own would leave the others inside a collective that never completes; found by the
    # world-2 CPU rehearsal of this function, tests/test_streams.py)
    transport, note = "rccl", None
    cid = [None]
    if rank == 0:
        try:
            cid = [h.comm_unique_id()]
        except Exception as e:                                   # noqa: BLE001
            cid = [None]
            note = f"dfd_comm_unique_id failed: {e}"
    if dist is not None:
        dist.broadcast_object_list(cid, src=0)
    ok = cid[0] is not None and not REHEARSE                   # (ranks that share a device cannot form an RCCL communicator)
    if ok:
        try:
            h.comm_init(cid[0], rank, world)
        except Exception as e:                                   # noqa: BLE001 - any failure -> documented fallback
            ok, note = False, f"dfd_comm_init failed: {e}"
    if dist is not None:
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=_red_dev(local_rank) if on_gpu else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        ok = bool(flag.item())
    if not ok:
        transport = "torch" if world > 1 else "local"
        note = note or "dfd_comm_init failed on another rank"
    # `extra_handles`: further handles on this rank's device - the look-ahead groups are computed two at a time (one per
    # handle, on host threads: ShardedStreams.local_records_groups), the exchange and the replay stay in wave order
    sh = S.ShardedStreams(h, n_streams, rank, world, transport=transport, extra_handles=extra_handles)
    h.warmup(min(n_streams * lookahead, h.max_batch), n_streams * lookahead)     # GEMM tiles of this batch shape (untimed)
    for e in extra_handles:
        e.tiles_import(h.tiles_export())
        e.warmup(min(n_streams * lookahead, e.max_batch), n_streams * lookahead)

    def batch(t):
        cur = [stream_frame(bases[s], t) for s in range(n_streams)]
        prev = [stream_frame(bases[s], t - 1) for s in range(n_streams)] if t > 0 else []
        return np.stack(cur + prev), [(s, t, t > 0) for s in range(n_streams)]

    # resident in HBM before the timed region: this rank's frames (and their predecessors), `lookahead` waves per device
    # batch (current frames of the group wave by wave, then their predecessors)
    staged = []
    for g0 in range(0, waves, lookahead):
        cur, prev, items = [], [], []
        for w in range(g0, min(g0 + lookahead, waves)):
            t = sh.frame_of(w)
            cur += [stream_frame(bases[s], t) for s in range(n_streams)]
            if t > 0:
                prev += [stream_frame(bases[s], t - 1) for s in range(n_streams)]
            items.append([(s, t, t > 0) for s in range(n_streams)])
        arr = np.stack(cur + prev)
        staged.append((h.alloc(arr.nbytes).upload(arr), items))
    # untimed warm-up on a throw-away driver (workspace growth, first-use costs), incl. one collective
    warm = S.ShardedStreams(h, n_streams, rank, world, transport=transport, extra_handles=extra_handles)
    par = len(warm.workers)
    # (the warm-up exchanges ONE group whatever `par` is: the number of collective calls must not depend on whether a rank
    # has its second handle)
    warm.finish_waves(warm.local_records_groups([(fd.ptr, Hh, Ww, items) for fd, items in staged[:par]])[0])
    fence()
    seq = {s: [] for s in range(n_streams)}
    t0 = time.perf_counter()
    for g0 in range(0, len(staged), par):
        # one device pass per look-ahead group, `par` groups side by side (one per handle)
        for blocks in sh.local_records_groups([(fd.ptr, Hh, Ww, items) for fd, items in staged[g0:g0 + par]]):
            for out in sh.finish_waves(blocks):                                  # one collective per wave, in wave order
                for s, rows in out.items():
                    seq[s] += [(r['frame'], r['confidence_level'], r['fake_probability']) for r in rows]
    fence()
    for e in extra_handles:
        e.sync()
    dt = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([dt], dtype=torch.float64, device=_red_dev(local_rank) if on_gpu else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    for fd, _ in staged:
        fd.free()
    frames = waves * world * n_streams
    res = {"workload": f"{n_streams} seeded {Hh}x{Ww} streams (seeds 100-107), frame t on rank t % {world}; per wave: SSD detect + "
                       "faces[0] -> CLAHE -> 224 -> B0, six forensic signals (temporal from recomputed gray(t-1)), one "
                       "all-gather of 80-byte records, replay of temporal score + votes on every rank; the frames of "
                       f"{lookahead} consecutive waves share one device batch (look-ahead) and one dfd_vote_allgather_waves call "
                       "(one upload / download / stream wait per group), the exchange itself stays one all-gather per wave",
           "frames_per_s": round(frames / dt, 1), "ms_per_wave": round(dt / waves * 1e3, 3), "waves": waves,
           "frames_per_wave_per_gpu": n_streams, "lookahead_waves": lookahead, "transport": transport,
           "groups_in_flight_per_gpu": par,
           "collective": "dfd_vote_allgather_waves (one ncclAllGather per wave, RCCL)" if transport == "rccl" else transport,
           "record_bytes": S.RECORD_FLOATS * 8, "bytes_gathered_per_wave": S.RECORD_FLOATS * 8 * n_streams * world}
    if note:
        res["transport_note"] = note
    # verdict-sequence equality with the single-GPU sequence (rank 0, untimed): every frame unless verify_frames caps it
    if rank == 0:
        nver = waves * world if verify_frames is None else min(verify_frames, waves * world)
        one = S.ShardedStreams(h, n_streams, 0, 1, transport="local")
        truth = {s: [] for s in range(n_streams)}
        for t in range(nver):
            arr, items = batch(t)
            fd = h.alloc(arr.nbytes).upload(arr)
            for s, rows in one.finish_wave(one.local_records(fd.ptr, Hh, Ww, items)).items():
                truth[s] += [(r['frame'], r['confidence_level'], r['fake_probability']) for r in rows]
            fd.free()
        same = all(seq[s][:nver] == truth[s] for s in range(n_streams))
        res["verdicts_equal_single_gpu"] = bool(same)
        res["verified_frames_per_stream"] = nver
        res["verdicts_stream0"] = [lv for _, lv, _ in seq[0]]
        if not same:                                             # the line is still printed; the run then exits non-zero
            res["error"] = "sharded verdict sequence differs from the single-GPU sequence"
    if transport == "rccl":
        h.comm_destroy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: instrumented steps (roofline, per-launch times), lane and oracle "
                         "checks, the other classifier loops and precisions, the 1080p end-to-end and stream extras, the "
                         "CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the logits of the last timed step to DIR/logits.npy (float32, batch x 1)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--layers", action="store_true", help="with --full: print the per-launch table to stderr")
    ap.add_argument("--no-e2e", action="store_true", help="with --full: skip the 1080p end-to-end extra (configs[2]/[3])")
    ap.add_argument("--no-streams", action="store_true", help="with --full: skip the frame-sharded 8-stream extra (configs[4])")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    # stdout carries exactly ONE line (the JSON): libraries that print there (RCCL's version banner at communicator
    # creation) are sent to stderr for the whole run; the JSON goes to the saved descriptor.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    json_out = os.fdopen(json_fd, "w")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            sys.exit("bench.py --gpus N>1 must be launched with torch.distributed.run (one rank per GPU)")
        args.gpus = world

    import torch

    import rtdfd_amd
    from rtdfd_amd import b0_arch

    dist = None
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if REHEARSE:
            local_rank = local_rank % max(torch.cuda.device_count(), 1)
            torch.cuda.set_device(local_rank)
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    sd = rtdfd_amd.weights.seeded_state_dict(0)
    blob = rtdfd_amd.weights.pack_all(sd, rtdfd_amd.weights.seeded_ssd_state_dict(0))
    h = rtdfd_amd._lib.Handle(blob, device=local_rank, max_batch=args.batch)

    # synthetic crops of configs[1]: torch.manual_seed(1); randn(256,3,224,224) (seed + rank on other ranks)
    g = torch.Generator().manual_seed(1 + rank)
    x = torch.randn(args.batch, 3, 224, 224, generator=g).numpy()
    xd = h.alloc(x.nbytes).upload(x)
    yd = h.alloc(args.batch * 4)

    def barrier():
        h.sync()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()
        h.sync()

    # dfd_warmup sizes the workspace, splits the weights and measures the GEMM tile of every layer shape at this batch
    # (classifier) and at the e2e extra's 64 frames (detector): the only place the library synchronises for tuning.
    h.warmup(args.batch, E2E_FRAMES if args.full and not args.no_e2e else 0)
    # TWO forwards in flight (rtdfd_amd._lib.ClassifierLanes: a second handle = its own stream and workspace, the same
    # weights and tile table) take the K steps in turn.  A step is still one batch-256 forward; the second forward's
    # kernels fill the launch gaps and under-filled late layers of the first.  DFD_BENCH_LANES=1 is
    # round 3's single-forward loop.
    lanes = rtdfd_amd._lib.ClassifierLanes(blob, device=local_rank, max_batch=args.batch, lanes=LANES, first=h)
    # (both lanes at normal priority: a high-priority stream made this early changes how the handle's low-priority second
    # stream is scheduled for the rest of the process - the forensic / JPEG rows lost their overlap, 11.9 -> 11.1 k and
    # 10.3 -> 8.8 k frames/s, even with the lane closed before them; DFD_BENCH_LANE_PRIORITY=1 tries it)
    if len(lanes) > 1 and os.environ.get("DFD_BENCH_LANE_PRIORITY", "0") == "1":
        lanes.handles[1].set_option("stream_priority", 1)
    lanes.warmup(args.batch)
    ys = [yd] + [h.alloc(args.batch * 4) for _ in range(len(lanes) - 1)]
    # untimed, before the warm-up steps: do the two lanes overlap in THIS process?  (after torch.distributed / RCCL have made
    # their streams the runtime may put both lanes on one hardware queue; the check then moves lane 1 to another pool)
    overlap = lanes.check_overlap(xd.ptr, args.batch, ys) if len(lanes) > 1 and os.environ.get("DFD_BENCH_LANE_PRIORITY") is None else None
    for i in range(max(args.warmup, 1)):
        lanes.submit(xd.ptr, args.batch, ys[i % len(lanes)].ptr)
    lanes.sync()
    lanes._next = 0
    barrier()
    # HIP events after every launch, on the library's stream, live in the timed region: on every step they cost 5 % of it
    # (3.85 vs 3.66 ms per batch-256 step), so every PROFILE_EVERY-th step carries them.  An instrumented step runs ALONE:
    # ClassifierLanes.submit_alone orders it on the device (dfd_wait_for: it starts when the other lane has finished its
    # step, the other lane's next step starts when it has finished; no host wait, so the host stays ahead of the GPU and
    # the gaps between its events are kernel time).  Its events then time isolated kernels, which is what the roofline
    # object must describe; the time the other lane idles beside it is inside the timed region and `value` pays for it.
    # Only a --full run instruments steps: a plain run times the two lanes and nothing else.
    nl = len(lanes)
    every, first = 0, args.steps
    if args.full:
        every = PROFILE_EVERY if args.steps >= PROFILE_EVERY else max(nl, args.steps // nl * nl)
        every = (every + nl - 1) // nl * nl                      # instrumented steps fall on lane 0 ...
        first = every // 2 // nl * nl                            # ... in the middle of each window of `every` steps
        h.set_option("profile_stride", every // nl)
    t0 = time.perf_counter()
    for i in range(args.steps):
        if i == first:
            h.profile_begin()                                    # host-side only: lane 0's next forward is sample 0
        if i >= first and (i - first) % every == 0:
            lanes.submit_alone(xd.ptr, args.batch, ys[i % nl].ptr)
        else:
            lanes.submit(xd.ptr, args.batch, ys[i % nl].ptr)
    lanes.sync()
    barrier()
    dt = time.perf_counter() - t0
    if args.full:
        steps_seen, layers = h.profile_end()
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device=_red_dev(local_rank))
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())

    crops = args.batch * args.steps * world
    value = crops / dt
    out = {
        "metric": "face-crops/sec (224x224 crops through EfficientNet-B0 classify)",
        "value": round(value, 1), "unit": "crops/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic (torch.manual_seed(1) randn crops, seeded random-init weights)",
        "config": {"workload": "configs[1]: batch=256 random 224x224 crops, EfficientNet-B0 fp32 inference",
                   "batch_per_gpu": args.batch, "parallelism": f"frame-shard x{world}, no data-path collective",
                   "forwards_in_flight": nl, "lanes_overlap_check_untimed": overlap,
                   "arithmetic": "fp32 storage and accumulation; 1x1-conv products are fp32-exact (each operand = exact sum "
                                 "of three bf16 terms, six cross terms on the bf16 MFMA; the dropped terms are < 2^-24 "
                                 "relative); DFD_SPLIT_GEMM=0 runs the same GEMMs on the fp32 MFMA instead"},
    }
    # what a caller of the timed path receives from its last step: that step's logits (lane (steps - 1) % lanes); the
    # inputs and weights are seeded, so two builds can be compared output for output
    if args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)
        last = ys[(args.steps - 1) % nl].download((args.batch, 1)).astype(np.float32)
        name = "logits.npy" if rank == 0 else f"logits_rank{rank}.npy"
        np.save(os.path.join(args.dump_outputs, name), last)

    if not args.full:
        if rank == 0:
            print(json.dumps(out), file=json_out, flush=True)
        for b in ys[1:]:
            b.free()
        lanes.close()
        xd.free()
        yd.free()
        h.close()
        if dist is not None:
            dist.destroy_process_group()
        return

    for k in range(1, min(nl, args.steps)):                      # every lane computed the same batch: the same bits
        if not np.array_equal(ys[k].download((args.batch, 1)), yd.download((args.batch, 1))):
            sys.exit(f"lane {k} logits differ from lane 0")
    logits = yd.download((args.batch, 1))
    if not np.all(np.isfinite(logits)):
        sys.exit("non-finite logits in the timed run")
    bf16_lanes = None
    if rank == 0 and world == 1 and nl > 1:
        bf16_lanes = bf16_two_lanes(lanes, xd, ys, args.batch, min(args.steps, 20) // nl * nl)
        h.warmup(args.batch, 0)                                  # (fp32 again: nothing to measure, the table has the entries)
    # the second lane is closed here: the rows below (other options, the 1080p extras with their copy / second compute
    # streams) run in a process that holds the first handle's streams only, as in the earlier rounds
    for b in ys[1:]:
        b.free()
    ys = ys[:1]
    lanes.close()
    # SURVEY 8(d) Config 2: parity on the first 8 rows of the timed run's own output, against the CPU oracle
    parity = None
    if rank == 0:
        from oracle import b0_ref

        want = b0_ref.forward(rtdfd_amd.weights.to_torch(sd), torch.from_numpy(x[:8])).numpy()
        parity = float(np.abs(logits[:8] - want).max())
        if not parity <= 1e-3:
            sys.exit(f"timed-run logits differ from the oracle: max|d| = {parity:.3e} > 1e-3")

    dw_ms = sum(ms for name, ms in layers if name.endswith(".dw")) / max(steps_seen, 1)
    all_ms = sum(ms for _, ms in layers) / max(steps_seen, 1)
    dw_bytes = b0_arch.depthwise_bytes_per_image() * args.batch       # per step = 16 launches
    achieved = dw_bytes / (dw_ms * 1e-3) / 1e9 if dw_ms > 0 else 0.0
    traffic, traffic_stamp, stamp_now = None, None, None
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    if os.path.exists(tpath):
        try:
            tj = json.load(open(tpath))
            traffic, traffic_stamp = tj.get("dw_hbm_bytes_per_step"), tj.get("stamp")
        except Exception:
            traffic = None
    try:
        sys.path.insert(0, os.path.join(ROOT, "profiles"))
        import source_stamp

        stamp_now = source_stamp.stamp()
    except Exception:
        stamp_now = None
    traffic_current = bool(traffic_stamp and stamp_now and
                           traffic_stamp.get("kernel_sources_sha16") == stamp_now.get("kernel_sources_sha16"))
    # bytes really moved (PMC) / the same launches' time: what the contract fraction cannot say once a launch carries more
    # than depthwise work (fused expand: the expanded tensor is never read, so traffic < algorithmic bytes)
    moved = traffic / (dw_ms * 1e-3) / 1e9 if (traffic and dw_ms > 0) else None

    # per depthwise launch: algorithmic bytes of that layer (input + output + k*k*C weights, fp32) / its duration
    per_layer = []
    for i, blk in enumerate(b0_arch.BLOCKS):
        ms = sum(m for name, m in layers if name == f"b{i}.dw") / max(steps_seen, 1)
        nbytes = (blk.h_in * blk.h_in + blk.h_out * blk.h_out + blk.kernel * blk.kernel) * blk.c_exp * 4 * args.batch
        if ms > 0:
            per_layer.append({"block": i, "k": blk.kernel, "stride": blk.stride, "hw": blk.h_in, "c_exp": blk.c_exp,
                              "us": round(ms * 1e3, 1), "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1),
                              "frac": round(nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 3)})

    out["config"]["instrumented_steps"] = (f"every {every}th step (from step {first}) carries per-launch HIP events and runs "
                                           "alone (the other lane waits for it on the device, inside the timed region): "
                                           "roofline durations are those of isolated kernels")
    out.update({
        "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                     # the contract's fraction prices ALGORITHMIC depthwise bytes (25.11 MB per crop) against the 16 launches'
                     # time; with the expand convs inside those launches (blocks 1-10, 12-15) their time also holds most of the
                     # net's 385 MMAC per crop, so beside it: the bytes the launches really moved (PMC) over the same time
                     "frac_bytes_moved": round(moved / HBM_PEAK_GBS, 4) if moved else None,
                     "achieved_bytes_moved": round(moved, 1) if moved else None,
                     "kernel": "the 16 depthwise launches per step: dfd::stem_dw_kernel (stem + block 0), dfd::mbconv_kernel / "
                               "mbconv2_kernel (blocks 1-5: 1x1 expand + depthwise), dfd::mbconv_late_kernel (blocks 6, 7, 10, 12-15: "
                               "expand + depthwise of whole images; option fuse_late, default on, per block where it measures "
                               "faster), dfd::dw_kernel / dw_rows7_kernel (blocks 8, 9, 11)",
                     "algorithmic_bytes_per_step": dw_bytes, "ms_per_step": round(dw_ms, 4),
                     "share_of_step": round(dw_ms / all_ms, 4) if all_ms else None,
                     "traffic_source": "profiles/traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of "
                                       "profiles/b0_profile_driver.py; counters cannot be read inside the run)",
                     "traffic_stamp": traffic_stamp, "stamp_of_this_run": stamp_now,
                     "traffic_measured_on_these_kernel_sources": traffic_current,
                     "per_layer": per_layer},
        "kernel_ms_per_step": round(all_ms, 3),
        "parity": {"rows": 8, "max_abs_logit_err_vs_oracle": parity, "tol": 1e-3},
    })
    if rank == 0 and world == 1:
        out["ms_by_kind"] = {k: round(sum(ms for n_, ms in layers if n_.split(".")[-1] == k) / max(steps_seen, 1), 3)
                             for k in ("dw", "se", "proj", "exp", "head", "avgpool", "mlp")}
        out["fuse_late_off"] = separate_late_launches(h, xd, yd, args.batch, min(args.steps, 20), logits)
        out["one_forward_in_flight"] = one_forward_in_flight(h, xd, yd, args.batch, min(args.steps, 20), logits)
        out["bf16"] = bf16_classify(h, xd, yd, args.batch, min(args.steps, 20), logits, b0_arch.depthwise_bytes_per_image(2) * args.batch)
        if bf16_lanes:
            out["bf16"]["two_forwards_in_flight"] = bf16_lanes
    if not args.no_e2e:
        out["e2e"] = e2e_frames(h, rank, dist, local_rank, blob=blob)
    if not args.no_streams:
        # the extra must never cost the main line: if the collective set-up wedges, rank 0 prints what it has
        import threading

        def bail():
            if rank == 0:
                out["config5"] = {"error": "timed out after 240 s (collective set-up?)"}
                print(json.dumps(out), file=json_out, flush=True)
            os._exit(3)                                          # the partial line is out; a wedged run is not a success

        guard = threading.Timer(240.0, bail)
        guard.daemon = True
        guard.start()
        extra = []
        try:
            if os.environ.get("DFD_BENCH_STREAM_HANDLES", "2") != "1":
                # a second handle per rank for the look-ahead groups (its main stream from the high-priority pool, made
                # after every single-call row: DESIGN section 5).  A rank that cannot make it computes its groups one
                # after the other: same records, same collective calls.
                try:
                    e2 = rtdfd_amd._lib.Handle(blob, device=local_rank, max_batch=args.batch)
                    e2.set_option("stream_priority", 1)
                    extra.append(e2)
                except Exception as e:                           # noqa: BLE001
                    print(f"[bench] no second handle for the stream groups: {e}", file=sys.stderr)
            out["config5"] = config5_streams(h, rank, world, dist, local_rank, extra_handles=extra)
        except SystemExit:
            raise
        except Exception as e:                                   # noqa: BLE001
            out["config5"] = {"error": f"{type(e).__name__}: {e}"}
        guard.cancel()
        for e2 in extra:
            e2.close()
    if rank == 0:
        if args.layers:
            agg = {}
            for name, ms in layers:
                key = name.split(".")[-1] if "." in name else name
                agg[key] = agg.get(key, 0.0) + ms / max(steps_seen, 1)
            print("per-launch ms/step:", file=sys.stderr)
            for name, ms in layers:
                print(f"  {name:10s} {ms / max(steps_seen, 1):8.4f}", file=sys.stderr)
            print("by kind:", {k: round(v, 3) for k, v in agg.items()}, file=sys.stderr)
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(sd, with_e2e=not args.no_e2e)
        print(json.dumps(out), file=json_out, flush=True)
    xd.free()
    yd.free()
    h.close()
    if dist is not None:
        dist.destroy_process_group()
    if rank == 0 and isinstance(out.get("config5"), dict) and out["config5"].get("verdicts_equal_single_gpu") is False:
        sys.exit("config5: sharded verdict sequence differs from the single-GPU sequence")


if __name__ == "__main__":
    main()
