"""Stage benches beside bench.py's headline line: one JSON line per stage.

  vit       BASELINE config 4: ViT-L/16 (or -B) encoder-only, enc-batch 128 over pre-cropped
            224x224 uint8 faces resident in HBM (blob 224 -> 128 + ViT forward; split-fp16 or fp32 MFMA);
            roofline = encoder FLOPs (39.78 / 11.27 GFLOP per face) / step time.
  grouping  the grouping step on N planted-cluster embeddings (N=10k, D=512 by default):
            fused cosine dedupe (dupes.py:51-68) and the KMeans + silhouette/CH/DB sweep
            (grouping.py:92-137) for k = 2..16, each timed with a device sync on both sides.
  jpeg      the face-file write of one det-batch (detection.py:155-158): 16 device-generated 720p
            frames, the crops detect_crops gives for them (MTCNN; a fixed list of 48 rectangles of
            100-250 px when that yields fewer than 16), quality 95.  Two legs in one process:
            host = one .cpu().numpy() slice per crop + utils.imwrite (the jpeg_encoder='host'
            path), device = utils.jpeg_encode_crops + writing the same files.  ms per det-batch,
            the ratio and the bytes each moves D2H.
  resize    the same det-batch written with resize_to=160 (detection.py:147-158): jpeg's frames and
            rectangles.  host = one .cpu().numpy() slice per crop + utils.resize_keep_ratio +
            dupes.ahash of the resized face (an upload and a launch per face) + utils.imwrite,
            device = utils.resize_crops + dupes.ahash_crops + utils.jpeg_encode_crops on the atlas +
            writing the files; resize_only = utils.resize_crops alone.  ms per det-batch, the
            copies and bytes each moves, and whether the two legs wrote the same files.
  jpeg_decode  the face-file read of the grouping stage (grouping.py:29-40): about 1,024 face files
            written by the device encoder from device-generated 720p frames and the crops
            detect_crops gives for them.  Two legs in one process: host = encode_faces' path up to
            the uploaded buffer (_imread of every file, pad into [n,Hmax,Wmax,3], one H2D copy per
            enc-batch of 16), device = reading the bytes + utils.jpeg_decode in groups of
            grouping.DECODE_GROUP files.  ms per 1,024 files (scaled when fewer files), the ratio,
            the bytes each moves H2D and the two kernel stages by HIP events.
  handoff   the face hand-off from detection to grouping (face_handoff='device'): jpeg_decode's
            inputs, encoded with decoded=True so that a FaceStore holds every face's decoded pixels
            in HBM.  Three legs in one process, each up to the atlas in HBM: host = jpeg_decode's
            host leg, device = reading the bytes + utils.jpeg_decode, store = utils.faces_to_atlas
            from the store, in groups of grouping.DECODE_GROUP (no file opened).  ms per 1,024
            faces and the ratios; also the encode call of one det-batch with decoded=False and
            decoded=True (the surcharge the detection stage pays for the stored pixels).
  mjpeg     reading one det-batch of a Motion-JPEG file (video.MJPEGReader): 16 device-generated
            720p frames, encoded once with Pillow at quality 90 into an AVI file.  Three legs in one
            process, each from the memory-mapped file to BGR frames in HBM: host = read(decoder=
            'host') (Pillow on one core + one upload), serial = utils.jpeg_decode(scan='serial') on
            the frames' bytes (one lane per frame), device = read(decoder='device')
            (vtf_jpeg_decode_split).  ms per det-batch, the ratios, the device leg's two kernel
            stages by HIP events and a seg_bytes sweep (64, 128, 256, 512).

The CPU legs are the oracle (ViT torch-CPU restatement) and sklearn 1.7.2 itself (the
reference's own grouping dependency), on bounded samples, timed on this host's cores.

  python scripts/bench_stages.py vit [--vit-model vit_l] [--steps 10] [--warmup 2]
  python scripts/bench_stages.py grouping [--n 10000] [--d 512]
  python scripts/bench_stages.py jpeg [--steps 20] [--warmup 3]
  python scripts/bench_stages.py resize [--steps 20] [--warmup 3]
  python scripts/bench_stages.py jpeg_decode [--steps 10] [--warmup 3]
  python scripts/bench_stages.py handoff [--steps 10] [--warmup 3]
  python scripts/bench_stages.py mjpeg --steps 20 --warmup 3
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'video-to-faces_amd')]

import numpy as np  # noqa: E402
import torch  # noqa: E402

FP32_PEAK_TFLOPS = 157.3  # MI355X dense fp32 MFMA (MI355X_MICROARCH.md)
F16X_PEAK_TFLOPS = round(2500.0 / 3, 1)  # fp16 dense MFMA / 3 products (split-fp16 operands)
VIT_GFLOP = {'vit_b': 11.27, 'vit_l': 39.78}  # per face at 128x128


def cores():
    n = len(os.sched_getaffinity(0))
    env = os.environ.get('OMP_NUM_THREADS')
    return min(n, int(env)) if env and env.isdigit() else n


def bench_vit(a):
    from videotofaces import synth
    from videotofaces.encoders.vit import ViT
    isL = a.vit_model == 'vit_l'
    dev = torch.device('cuda:0')
    params = synth.make_params(a.vit_model)
    m = ViT(dev, params, isL=isL, precision=a.vit_precision)
    B = a.enc_batch
    crops_u8 = torch.from_numpy(synth.make_crops(B, 224, seed=1)).to(dev)  # [B,224,224,3] in HBM
    boxes = np.array([[i, 0, 0, 224, 224] for i in range(B)], np.int32)
    stream = torch.cuda.current_stream(dev)
    for _ in range(a.warmup):
        m.encode_crops(crops_u8, boxes)
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(stream)
    for _ in range(a.steps):
        out = m.encode_crops(crops_u8, boxes)
    e1.record(stream)
    torch.cuda.synchronize(dev)
    wall = time.perf_counter() - t0
    ms = e0.elapsed_time(e1) / a.steps
    assert out.shape == (B, m.dim) and bool(torch.isfinite(out).all())
    achieved = VIT_GFLOP[a.vit_model] * B / ms  # GFLOP/ms = TFLOP/s
    # split-fp16: three fp16 products per fp32-grade product -> fp16 dense peak / 3
    peak = FP32_PEAK_TFLOPS if a.vit_precision == 'fp32' else F16X_PEAK_TFLOPS
    res = {'metric': 'faces/sec, %s encoder on pre-cropped 224x224 faces (BASELINE config 4)' % a.vit_model,
           'value': round(a.steps * B / wall, 2), 'unit': 'faces/s', 'n_gpus': 1, 'steps': a.steps,
           'warmup': a.warmup, 'ms_per_step': round(wall * 1e3 / a.steps, 3), 'higher_is_better': True,
           'dtype': 'fp32' if a.vit_precision == 'fp32' else 'fp32 (split-fp16 MFMA, guarded)', 'data': 'synthetic (seeded 224x224 crops, hash-seeded weights)',
           'config': {'workload': '%s enc-batch %d, 224x224 uint8 crops in HBM -> blob 128x128 -> ViT'
                                  % (a.vit_model, B), 'enc_batch': B},
           'roofline': {'kernel': 'whole encoder step (blob + %d k_conv GEMM launches + attention + LN)'
                                  % (12 * (2 if isL else 1) * 4 + 2),
                        'bound': 'mfma', 'achieved': round(achieved, 3), 'peak': peak,
                        'unit': 'TFLOP/s', 'frac': round(achieved / peak, 4),
                        'gflop_per_face': VIT_GFLOP[a.vit_model], 'event_ms_per_step': round(ms, 3)},
           'cpu_baseline': None}
    if not a.no_cpu_baseline:
        from oracle.vit import vit
        torch.set_num_threads(cores())
        n = a.cpu_faces
        x = (torch.from_numpy(synth.make_crops(n, 128, seed=2)).permute(0, 3, 1, 2).float() - 127.5) / 127.5
        dim, depth = (1024, 24) if isL else (768, 12)
        vit(params, x[:1], dim, depth)  # warm-up
        t0 = time.time()
        vit(params, x, dim, depth)
        dt = time.time() - t0
        res['cpu_baseline'] = {'value': round(n / dt, 3), 'unit': 'faces/s', 'cores': cores(), 'kind': 'port',
                               'sample': '%d faces at 128x128, oracle %s forward fp32 on CPU, %.1f s'
                                         % (n, a.vit_model, dt)}
    print(json.dumps(res), flush=True)


def bench_grouping(a):
    from videotofaces import synth, dupes
    from videotofaces.grouping import cluster_sweep
    dev = torch.device('cuda:0')
    X = synth.planted_clusters(a.n, a.d, seed=0)
    Xd = torch.from_numpy(X).to(dev)
    ks = list(range(2, a.kmax + 1))
    dupes.cosine_dedupe_device(Xd[:256])  # warm-up (library load, scratch)
    cluster_sweep(X[:512], [2], 0)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    mins, inds = dupes.cosine_dedupe_device(Xd)
    torch.cuda.synchronize(dev)
    t_dd = time.perf_counter() - t0
    t0 = time.perf_counter()
    labels, scores = cluster_sweep(X, ks, 0)
    torch.cuda.synchronize(dev)
    t_sw = time.perf_counter() - t0
    best_k = scores[int(np.argmax([s[1] for s in scores]))][0]
    cos_tflop = a.n * a.n * a.d / 1e12  # lower-triangle GEMM, 2 FLOP per MAC
    res = {'metric': 'grouping time (cosine dedupe + KMeans/silhouette/CH/DB sweep k=2..%d)' % a.kmax,
           'value': round(t_dd + t_sw, 4), 'unit': 's', 'higher_is_better': False, 'n_gpus': 1,
           'dtype': 'fp32 (KMeans bit-exact labels, scores f64)',
           'data': 'synthetic planted clusters (8 centres, sigma 0.5, seed 0)',
           'config': {'workload': 'N=%d D=%d' % (a.n, a.d), 'N': a.n, 'D': a.d, 'k': [ks[0], ks[-1]]},
           'dedupe_s': round(t_dd, 4), 'sweep_s': round(t_sw, 4), 'sweep_s_per_k': round(t_sw / len(ks), 4),
           'best_k_silhouette': int(best_k), 'dupes_at_0.25': int((mins <= 0.25).sum()),
           'dedupe_roofline': {'bound': 'mfma', 'achieved': round(cos_tflop / t_dd, 3), 'peak': FP32_PEAK_TFLOPS,
                               'unit': 'TFLOP/s', 'frac': round(cos_tflop / t_dd / FP32_PEAK_TFLOPS, 4)},
           'cpu_baseline': None}
    if not a.no_cpu_baseline:
        import sklearn.cluster
        import sklearn.metrics
        from oracle import grouping as og
        torch.set_num_threads(cores())
        t0 = time.time()
        og.cosine_dedupe(X)
        c_dd = time.time() - t0
        kc = ks[:a.cpu_ks]
        t0 = time.time()
        for k in kc:
            lb = sklearn.cluster.KMeans(n_clusters=k, random_state=0, n_init='auto').fit_predict(X)
            sklearn.metrics.silhouette_score(X, lb)
            sklearn.metrics.calinski_harabasz_score(X, lb)
            sklearn.metrics.davies_bouldin_score(X, lb)
        c_k = (time.time() - t0) / len(kc)
        res['cpu_baseline'] = {'value': round(c_dd + c_k * len(ks), 3), 'unit': 's', 'cores': cores(),
                               'kind': 'reference',
                               'sample': 'sklearn 1.7.2 (the reference\'s grouping dependency): cosine dedupe '
                                         '%.2f s at N=%d + %.2f s per k measured on k=%s, scaled to %d k'
                                         % (c_dd, a.n, c_k, kc, len(ks))}
    print(json.dumps(res), flush=True)


def jpeg_inputs():
    """The det-batch of the jpeg and resize stages -> (frames in HBM, rectangles, where they come from)"""
    from videotofaces import synth
    from videotofaces.detection import detect_crops
    from videotofaces.detectors.mtcnn import RealMTCNN
    dev = torch.device('cuda:0')
    B, H, W = 16, 720, 1280
    frames = synth.make_frames_device(0, B, H, W, seed=0, device=dev, style='blobs')
    import contextlib
    with contextlib.redirect_stdout(sys.stderr):  # (the model announces itself; stdout is the JSON line)
        model = RealMTCNN(dev)
    with torch.inference_mode():
        d_crops, _ = detect_crops(model, frames, 0)
    rects = d_crops.cpu().numpy()
    source = 'detect_crops (MTCNN, default box settings)'
    if len(rects) < 16:
        rng = np.random.default_rng(0)
        rects = []
        for i in range(48):
            w, h = int(rng.integers(100, 251)), int(rng.integers(100, 251))
            x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
            rects.append([i % B, x, y, x + w, y + h])
        rects = np.array(rects, np.int32)
        source = 'fixed list (seeded): 48 rectangles of 100-250 px'
    return frames, rects, source


def bench_jpeg(a):
    import tempfile
    from videotofaces.utils import imwrite, jpeg_encode_crops
    frames, rects, source = jpeg_inputs()
    dev = frames.device
    n = len(rects)
    names = ['%06d.jpg' % i for i in range(n)]

    def host_leg(d):
        for (fi, x1, y1, x2, y2), fn in zip(rects.tolist(), names):
            imwrite(os.path.join(d, fn), np.ascontiguousarray(frames[fi][y1:y2, x1:x2].cpu().numpy()))

    def device_leg(d):
        for data, fn in zip(jpeg_encode_crops(frames, rects, 95), names):
            with open(os.path.join(d, fn), 'wb') as f:
                f.write(data)

    def encode_only(d):
        jpeg_encode_crops(frames, rects, 95)

    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for leg, fn in (('host', host_leg), ('device', device_leg), ('device_encode_only', encode_only)):
            d = os.path.join(tmp, leg)
            os.makedirs(d)
            for _ in range(a.warmup):
                fn(d)
            torch.cuda.synchronize(dev)
            ts = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                fn(d)
                torch.cuda.synchronize(dev)
                ts.append((time.perf_counter() - t0) * 1e3)
            out[leg] = ts
        sizes = {leg: sum(os.path.getsize(os.path.join(tmp, leg, f)) for f in names) for leg in ('host', 'device')}
    try:
        import cv2  # noqa: F401
        writer = 'cv2.imwrite'
    except ImportError:
        writer = 'Pillow save(quality=95)'
    pix = int(((rects[:, 3] - rects[:, 1]).astype(np.int64) * (rects[:, 4] - rects[:, 2])).sum())
    med = {k: float(np.median(v)) for k, v in out.items()}
    res = {'metric': 'face JPEG write, ms per det-batch (16 x 720p frames, %d crops, quality 95)' % n,
           'value': round(med['device'], 3), 'unit': 'ms', 'higher_is_better': False, 'n_gpus': 1,
           'steps': a.steps, 'warmup': a.warmup, 'data': 'synthetic (device-generated blobs frames, seed 0)',
           'config': {'crops': n, 'crop_source': source, 'crop_pixels': pix, 'host_writer': writer,
                      'host_cores_used': 1},
           'host_ms': round(med['host'], 3), 'host_ms_min': round(min(out['host']), 3),
           'device_ms': round(med['device'], 3), 'device_ms_min': round(min(out['device']), 3),
           'device_encode_only_ms': round(med['device_encode_only'], 3),
           'host_over_device': round(med['host'] / med['device'], 2),
           'd2h_bytes': {'host': pix * 3, 'device': sizes['device']},
           'd2h_copies': {'host': n, 'device': 1},
           'file_bytes': sizes, 'files_identical_size': sizes['host'] == sizes['device']}
    print(json.dumps(res), flush=True)


def bench_resize(a):
    import tempfile
    from videotofaces.dupes import ahash, ahash_crops
    from videotofaces.utils import imwrite, jpeg_encode_crops, resize_crops, resize_keep_ratio, resize_sizes
    to = 160
    frames, rects, source = jpeg_inputs()
    dev = frames.device
    n = len(rects)
    names = ['%06d.jpg' % i for i in range(n)]

    def host_leg(d):  # process_frames_batch with resize_to before the device path took it
        faces = [resize_keep_ratio(frames[fi][y1:y2, x1:x2].cpu().numpy(), to) for fi, x1, y1, x2, y2 in rects.tolist()]
        hs = [ahash(img, dev) for img in faces]
        for img, fn in zip(faces, names):
            imwrite(os.path.join(d, fn), np.ascontiguousarray(img))
        return hs

    def device_leg(d):
        atlas, sizes = resize_crops(frames, rects, to)
        slots = np.zeros((n, 5), np.int32)
        slots[:, 0], slots[:, 3], slots[:, 4] = np.arange(n), sizes[:, 1], sizes[:, 0]
        hs = ahash_crops(atlas, slots)
        for data, fn in zip(jpeg_encode_crops(atlas, slots, 95), names):
            with open(os.path.join(d, fn), 'wb') as f:
                f.write(data)
        return hs

    def resize_only(d):
        resize_crops(frames, rects, to)

    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for leg, fn in (('host', host_leg), ('device', device_leg), ('resize_only', resize_only)):
            d = os.path.join(tmp, leg)
            os.makedirs(d)
            for _ in range(a.warmup):
                fn(d)
            torch.cuda.synchronize(dev)
            ts = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                fn(d)
                torch.cuda.synchronize(dev)
                ts.append((time.perf_counter() - t0) * 1e3)
            out[leg] = ts
        files = {leg: [open(os.path.join(tmp, leg, f), 'rb').read() for f in names] for leg in ('host', 'device')}
    try:
        import cv2  # noqa: F401
        writer = 'cv2.imwrite'
    except ImportError:
        writer = 'Pillow save(quality=95)'
    pix = int(((rects[:, 3] - rects[:, 1]).astype(np.int64) * (rects[:, 4] - rects[:, 2])).sum())
    dst = np.asarray(resize_sizes([(r[4] - r[2], r[3] - r[1]) for r in rects.tolist()], to), np.int64)
    dpix = int((dst[:, 0] * dst[:, 1]).sum())
    med = {k: float(np.median(v)) for k, v in out.items()}
    fbytes = {leg: sum(len(f) for f in v) for leg, v in files.items()}
    res = {'metric': 'resized face write, ms per det-batch (16 x 720p frames, %d crops, resize_to %d, hashes, '
                     'quality 95)' % (n, to),
           'value': round(med['device'], 3), 'unit': 'ms', 'higher_is_better': False, 'n_gpus': 1,
           'steps': a.steps, 'warmup': a.warmup, 'data': 'synthetic (device-generated blobs frames, seed 0)',
           'config': {'crops': n, 'crop_source': source, 'crop_pixels': pix, 'resize_to': to, 'resized_pixels': dpix,
                      'atlas_bytes': int(n * dst[:, 0].max() * dst[:, 1].max() * 3), 'host_writer': writer,
                      'host_cores_used': 1},
           'host_ms': round(med['host'], 3), 'host_ms_min': round(min(out['host']), 3),
           'device_ms': round(med['device'], 3), 'device_ms_min': round(min(out['device']), 3),
           'resize_only_ms': round(med['resize_only'], 3), 'resize_only_ms_min': round(min(out['resize_only']), 3),
           'host_over_device': round(med['host'] / med['device'], 2),
           # host: a slice and a hash word per crop; device: the hash words and the files' bytes
           'd2h_copies': {'host': 2 * n, 'device': 2},
           'd2h_bytes': {'host': pix * 3 + 8 * n, 'device': 8 * n + fbytes['device']},
           'h2d_pixel_copies': {'host': n, 'device': 0}, 'h2d_pixel_bytes': {'host': dpix * 3, 'device': 0},
           'file_bytes': fbytes, 'files_identical': files['host'] == files['device'],
           'whole_run_measured': False}
    print(json.dumps(res), flush=True)


def bench_jpeg_decode(a):
    import contextlib
    import tempfile
    from videotofaces import _native as nat
    from videotofaces import grouping, synth
    from videotofaces.detection import detect_crops
    from videotofaces.detectors.mtcnn import RealMTCNN
    from videotofaces.utils import jpeg_decode, jpeg_encode_crops
    dev = torch.device('cuda:0')
    B, H, W, want, bs = 16, 720, 1280, 1024, 16
    with contextlib.redirect_stdout(sys.stderr):
        model = RealMTCNN(dev)
    files, source = [], 'detect_crops (MTCNN, default box settings)'
    rng = np.random.default_rng(0)
    for seed in range(64):
        frames = synth.make_frames_device(0, B, H, W, seed=seed, device=dev, style='blobs')
        with torch.inference_mode():
            d_crops, _ = detect_crops(model, frames, 0)
        rects = d_crops.cpu().numpy()
        if len(rects) < 16:
            rects = []
            for i in range(48):
                w, h = int(rng.integers(100, 251)), int(rng.integers(100, 251))
                x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
                rects.append([i % B, x, y, x + w, y + h])
            rects = np.array(rects, np.int32)
            source = 'fixed list (seeded): rectangles of 100-250 px'
        files += jpeg_encode_crops(frames, rects, 95)
        if len(files) >= want:
            break
    files = files[:want]
    n = len(files)
    del frames
    group = grouping.DECODE_GROUP

    def host_leg(paths):
        moved = 0
        for at in range(0, n, bs):
            images = [grouping._imread(p) for p in paths[at:at + bs]]
            hm, wm = max(im.shape[0] for im in images), max(im.shape[1] for im in images)
            buf = np.zeros((len(images), hm, wm, 3), np.uint8)
            for i, im in enumerate(images):
                buf[i, :im.shape[0], :im.shape[1]] = im
            torch.from_numpy(buf).to(dev)
            moved += buf.nbytes
        return moved

    stage_ms = np.zeros(2, np.float32)

    def device_leg(paths):
        moved, st = 0, np.zeros(2)
        for at in range(0, n, group):
            data = []
            for p in paths[at:at + group]:
                with open(p, 'rb') as f:
                    data.append(f.read())
            atlas, sizes, status = jpeg_decode(data, dev)
            assert not status.any()
            moved += sum(len(d) for d in data)
            nat.check(nat.lib().vtf_jpeg_decode_profile(1, stage_ms.ctypes.data))
            st += stage_ms
        device_leg.stages.append(st)
        return moved
    device_leg.stages = []

    out, moved = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, '%06d.jpg' % i) for i in range(n)]
        for p, data in zip(paths, files):
            with open(p, 'wb') as f:
                f.write(data)
        # the two paths give the same pixels
        atlas, sizes, status = jpeg_decode(files[:64], dev)
        got = atlas.cpu().numpy()
        for i in range(64):
            im = grouping._imread(paths[i])
            assert status[i] == 0 and np.array_equal(got[i, :im.shape[0], :im.shape[1]], im), i
        nat.check(nat.lib().vtf_jpeg_decode_profile(1, None))
        for leg, fn in (('host', host_leg), ('device', device_leg)):
            for _ in range(a.warmup):
                fn(paths)
            torch.cuda.synchronize(dev)
            device_leg.stages = []
            ts = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                moved[leg] = fn(paths)
                torch.cuda.synchronize(dev)
                ts.append((time.perf_counter() - t0) * 1e3)
            out[leg] = ts
        nat.check(nat.lib().vtf_jpeg_decode_profile(0, None))
    try:
        import cv2  # noqa: F401
        reader = 'cv2.imread'
    except ImportError:
        reader = 'Pillow open().convert(RGB)'
    scale = 1024.0 / n
    med = {k: float(np.median(v)) * scale for k, v in out.items()}
    stages = np.median(np.array(device_leg.stages), axis=0) * scale
    res = {'metric': 'face JPEG read for grouping, ms per 1024 files (quality 95, crops of 720p frames)',
           'value': round(med['device'], 3), 'unit': 'ms', 'higher_is_better': False, 'n_gpus': 1,
           'steps': a.steps, 'warmup': a.warmup, 'data': 'synthetic (device-generated blobs frames, device-encoded)',
           'config': {'files': n, 'crop_source': source, 'file_bytes': sum(len(f) for f in files),
                      'host_reader': reader, 'host_cores_used': 1, 'host_enc_batch': bs, 'device_group': group},
           'host_ms': round(med['host'], 3), 'host_ms_min': round(min(out['host']) * scale, 3),
           'device_ms': round(med['device'], 3), 'device_ms_min': round(min(out['device']) * scale, 3),
           'device_stage1_entropy_ms': round(float(stages[0]), 3),
           'device_stage2_pixels_ms': round(float(stages[1]), 3),
           'host_over_device': round(med['host'] / med['device'], 2),
           'h2d_bytes': moved, 'h2d_copies': {'host': -(-n // bs), 'device': -(-n // group)}}
    print(json.dumps(res), flush=True)


def bench_handoff(a):
    import contextlib
    import tempfile
    from videotofaces import grouping, synth
    from videotofaces.detection import detect_crops
    from videotofaces.detectors.mtcnn import RealMTCNN
    from videotofaces.facestore import FaceStore
    from videotofaces.utils import faces_to_atlas, jpeg_decode, jpeg_encode_crops
    dev = torch.device('cuda:0')
    B, H, W, want, bs = 16, 720, 1280, 1024, 16
    with contextlib.redirect_stdout(sys.stderr):
        model = RealMTCNN(dev)
    # jpeg_decode's inputs, encoded with decoded=True: the files and, per det-batch, a chunk of pixels
    files, chunks, source = [], [], 'detect_crops (MTCNN, default box settings)'
    rng = np.random.default_rng(0)
    first = None
    for seed in range(64):
        frames = synth.make_frames_device(0, B, H, W, seed=seed, device=dev, style='blobs')
        with torch.inference_mode():
            d_crops, _ = detect_crops(model, frames, 0)
        rects = d_crops.cpu().numpy()
        if len(rects) < 16:
            rects = []
            for i in range(48):
                w, h = int(rng.integers(100, 251)), int(rng.integers(100, 251))
                x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
                rects.append([i % B, x, y, x + w, y + h])
            rects = np.array(rects, np.int32)
            source = 'fixed list (seeded): rectangles of 100-250 px'
        if first is None:
            first = (frames, rects)
        fs, pixels, offsets, status = jpeg_encode_crops(frames, rects, 95, decoded=True)
        assert not status.any()
        chunks.append((len(files), pixels, offsets, np.stack([rects[:, 4] - rects[:, 2], rects[:, 3] - rects[:, 1]], 1)))
        files += fs
        if len(files) >= want:
            break
    files = files[:want]
    n = len(files)
    del frames
    group = grouping.DECODE_GROUP

    # the encode call of one det-batch, without and with the decoded pixels
    # (a call is a fraction of a millisecond: the two take turns, so that neither has the warmer clocks,
    # and ten times the steps of the legs)
    enc = {False: [], True: []}
    for step in range(-a.warmup, 10 * a.steps):
        for decoded in (False, True):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            jpeg_encode_crops(first[0], first[1], 95, decoded=decoded)
            torch.cuda.synchronize(dev)
            if step >= 0:
                enc[decoded].append((time.perf_counter() - t0) * 1e3)

    def host_leg(paths, store):
        moved = 0
        for at in range(0, n, bs):
            images = [grouping._imread(p) for p in paths[at:at + bs]]
            hm, wm = max(im.shape[0] for im in images), max(im.shape[1] for im in images)
            buf = np.zeros((len(images), hm, wm, 3), np.uint8)
            for i, im in enumerate(images):
                buf[i, :im.shape[0], :im.shape[1]] = im
            torch.from_numpy(buf).to(dev)
            moved += buf.nbytes
        return moved

    def device_leg(paths, store):
        moved = 0
        for at in range(0, n, group):
            data = []
            for p in paths[at:at + group]:
                with open(p, 'rb') as f:
                    data.append(f.read())
            atlas, sizes, status = jpeg_decode(data, dev)
            assert not status.any()
            moved += sum(len(d) for d in data)
        return moved

    def store_atlas(paths, store, at):
        ents = [store.get(p) for p in paths[at:at + group]]
        sizes = np.array([(h, w) for _, _, h, w in ents], np.int32)
        faces = [c[o:o + h * w * 3] for c, o, h, w in ents]
        return faces_to_atlas(faces, sizes, int(sizes[:, 0].max()), int(sizes[:, 1].max()), dev), sizes

    def store_leg(paths, store):
        for at in range(0, n, group):
            store_atlas(paths, store, at)
        return 0

    out, moved = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, '%06d.jpg' % i) for i in range(n)]
        for p, data in zip(paths, files):
            with open(p, 'wb') as f:
                f.write(data)
        store = FaceStore()
        for at, pixels, offsets, sizes in chunks:
            k = max(0, min(len(sizes), n - at))
            assert store.add(paths[at:at + k], pixels, offsets[:k], sizes[:k])
        assert len(store) == n
        # the store path gives the decoder's pixels
        atlas, sizes = store_atlas(paths, store, 0)
        ref, rsz, status = jpeg_decode(files[:group], dev)
        assert not status.any() and np.array_equal(sizes, rsz)
        for i in range(len(sizes)):
            h, w = sizes[i]
            assert torch.equal(atlas[i, :h, :w], ref[i, :h, :w]), i
        del atlas, ref
        for leg, fn in (('host', host_leg), ('device', device_leg), ('store', store_leg)):
            for _ in range(a.warmup):
                fn(paths, store)
            torch.cuda.synchronize(dev)
            ts = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                moved[leg] = fn(paths, store)
                torch.cuda.synchronize(dev)
                ts.append((time.perf_counter() - t0) * 1e3)
            out[leg] = ts
        store_bytes = store.nbytes
    try:
        import cv2  # noqa: F401
        reader = 'cv2.imread'
    except ImportError:
        reader = 'Pillow open().convert(RGB)'
    scale = 1024.0 / n
    med = {k: float(np.median(v)) * scale for k, v in out.items()}
    e0, e1 = float(np.median(enc[False])), float(np.median(enc[True]))
    res = {'metric': 'face hand-off to grouping, ms per 1024 faces (quality 95, crops of 720p frames)',
           'value': round(med['store'], 3), 'unit': 'ms', 'higher_is_better': False, 'n_gpus': 1,
           'steps': a.steps, 'warmup': a.warmup, 'data': 'synthetic (device-generated blobs frames, device-encoded)',
           'config': {'faces': n, 'crop_source': source, 'file_bytes': sum(len(f) for f in files),
                      'store_bytes': store_bytes, 'chunks': len(chunks), 'host_reader': reader, 'host_cores_used': 1,
                      'host_enc_batch': bs, 'device_group': group},
           'host_ms': round(med['host'], 3), 'host_ms_min': round(min(out['host']) * scale, 3),
           'device_ms': round(med['device'], 3), 'device_ms_min': round(min(out['device']) * scale, 3),
           'store_ms': round(med['store'], 3), 'store_ms_min': round(min(out['store']) * scale, 3),
           'device_over_store': round(med['device'] / med['store'], 2),
           'host_over_store': round(med['host'] / med['store'], 2),
           'h2d_bytes': moved,
           'encode_call': {'crops': int(len(first[1])), 'steps': len(enc[True]), 'order': 'alternating', 'plain_ms': round(e0, 3), 'plain_ms_min': round(min(enc[False]), 3),
                           'decoded_ms': round(e1, 3), 'decoded_ms_min': round(min(enc[True]), 3),
                           'surcharge_ms': round(e1 - e0, 3), 'decoded_over_plain': round(e1 / e0, 3)}}
    print(json.dumps(res), flush=True)


def bench_mjpeg(a):
    import io
    import tempfile
    from PIL import Image
    from videotofaces import _native as nat
    from videotofaces import synth
    from videotofaces.utils import jpeg_decode
    from videotofaces.video import MJPEGReader, write_mjpeg_avi
    dev = torch.device('cuda:0')
    B, H, W, quality = 16, 720, 1280, 90
    frames = synth.make_frames_device(0, B, H, W, seed=0, device=dev, style='blobs').cpu().numpy()
    jpegs = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(buf, 'JPEG', quality=quality)
        jpegs.append(buf.getvalue())
    idx = list(range(B))
    stage_ms = np.zeros(2, np.float32)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'clip.avi')
        write_mjpeg_avi(path, jpegs, fps='25:1')
        r = MJPEGReader(path)
        # the three legs give the same frames
        want = r.read(idx, dev, 'host')
        assert torch.equal(r.read(idx, dev, 'device'), want)
        atlas, sizes, status = jpeg_decode([r.frame_bytes(i) for i in idx], dev)
        assert not status.any() and torch.equal(atlas, want)
        del atlas, want
        out = {'host': timed(lambda: r.read(idx, dev, 'host')),
               'serial': timed(lambda: jpeg_decode([r.frame_bytes(i) for i in idx], dev)),
               'device': timed(lambda: r.read(idx, dev, 'device'))}
        nat.check(nat.lib().vtf_jpeg_decode_profile(1, None))
        stages = []
        for _ in range(a.steps):
            r.read(idx, dev, 'device')
            nat.check(nat.lib().vtf_jpeg_decode_profile(1, stage_ms.ctypes.data))
            stages.append(stage_ms.copy())
        sweep = {}
        for seg in (64, 128, 256, 512):
            ts, st = timed(lambda: r.read(idx, dev, 'device', seg)), []
            for _ in range(a.steps):
                r.read(idx, dev, 'device', seg)
                nat.check(nat.lib().vtf_jpeg_decode_profile(1, stage_ms.ctypes.data))
                st.append(float(stage_ms[0]))
            sweep[str(seg)] = {'read_ms': round(float(np.median(ts)), 3), 'stage1_ms': round(float(np.median(st)), 3)}
        nat.check(nat.lib().vtf_jpeg_decode_profile(0, None))
        r.close()
    med = {k: float(np.median(v)) for k, v in out.items()}
    stages = np.median(np.array(stages), axis=0)
    res = {'metric': 'Motion-JPEG det-batch read, ms per 16 frames of 720p (Pillow quality 90) up to BGR frames in HBM',
           'value': round(med['device'], 3), 'unit': 'ms', 'higher_is_better': False, 'n_gpus': 1,
           'steps': a.steps, 'warmup': a.warmup, 'data': 'synthetic (device-generated blobs frames, Pillow-encoded)',
           'config': {'frames': B, 'height': H, 'width': W, 'quality': quality,
                      'file_bytes': sum(len(j) for j in jpegs), 'host_reader': 'Pillow open().convert(RGB)',
                      'host_cores_used': 1},
           'host_ms': round(med['host'], 3), 'host_ms_min': round(min(out['host']), 3),
           'serial_ms': round(med['serial'], 3), 'serial_ms_min': round(min(out['serial']), 3),
           'device_ms': round(med['device'], 3), 'device_ms_min': round(min(out['device']), 3),
           'device_stage1_entropy_ms': round(float(stages[0]), 3),
           'device_stage2_pixels_ms': round(float(stages[1]), 3),
           'host_over_device': round(med['host'] / med['device'], 2),
           'serial_over_device': round(med['serial'] / med['device'], 2),
           'seg_bytes_sweep': sweep}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('stage', choices=['vit', 'grouping', 'jpeg', 'resize', 'jpeg_decode', 'handoff', 'mjpeg'])
    ap.add_argument('--vit-model', default='vit_l', choices=['vit_b', 'vit_l'])
    ap.add_argument('--vit-precision', default='f16x', choices=['fp32', 'f16x'])
    ap.add_argument('--enc-batch', type=int, default=128)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--cpu-faces', type=int, default=16)
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--d', type=int, default=512)
    ap.add_argument('--kmax', type=int, default=16)
    ap.add_argument('--cpu-ks', type=int, default=3)
    ap.add_argument('--no-cpu-baseline', action='store_true')
    a = ap.parse_args()
    {'vit': bench_vit, 'grouping': bench_grouping, 'jpeg': bench_jpeg, 'resize': bench_resize,
     'jpeg_decode': bench_jpeg_decode, 'handoff': bench_handoff, 'mjpeg': bench_mjpeg}[a.stage](a)


if __name__ == '__main__':
    main()
