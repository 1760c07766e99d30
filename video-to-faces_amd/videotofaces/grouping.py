"""Encoding and grouping (drop-in for src/videotofaces/grouping.py).

classify (grouping.py:50-66) runs its cosine distances / argmin on the GPU
(vtf_cosine_classify).  cluster_faces (grouping.py:92-137) runs KMeans and the three
scores per k on the GPU (videotofaces.kmeans.Grouper, sklearn-faithful); under
torch.distributed the k sweep is sharded across ranks and the per-k labels
and scores are all-gathered.
"""
import collections
import math
import os
import os.path as osp
import shutil

import numpy as np
import torch

from . import _native as nat
from . import utils
from .dupes import remove_dupes_overall  # noqa: F401  (re-export like the reference)


def get_encoder_model(style, enc_model, device):
    """grouping.py:19-26 (style coupling kept: anime -> ViT, live -> FaceNet)."""
    if style == 'anime':
        from .encoders.vit import AnimeVIT
        isL = False if enc_model == 'default' else enc_model[-1] == 'l'
        return AnimeVIT(device, isL)
    if style == 'live':
        from .encoders.facenet import FaceNet
        isC = False if enc_model == 'default' else enc_model.split('_')[1] == 'casia'
        return FaceNet(device, isC)
    return 0


def _imread(p):
    try:
        import cv2
        return cv2.imread(p)
    except ImportError:
        from PIL import Image
        return np.asarray(Image.open(p).convert('RGB'))[:, :, ::-1].copy()


# jpeg_decoder='device': files per vtf_jpeg_decode call, the atlas bytes one call may take and the
# longest side a file may have in a shared atlas (a larger one is decoded on the host and makes a
# group of its own, so it does not enlarge the slots of other files)
DECODE_GROUP = 512
DECODE_ATLAS_BYTES = 1 << 30
DECODE_MAX_SIDE = 1024


def _area_rect(h, w, area):
    """crop_to_area's slice of an h x w image as (x1, y1, x2, y2), clipped as numpy clips it."""
    px1, py1, px2, py2 = area
    x1, x2, _ = slice(int(px1 * w), int(px2 * w + 1)).indices(w)
    y1, y2, _ = slice(int(py1 * h), int(py2 * h + 1)).indices(h)
    return x1, y1, max(x1, x2), max(y1, y2)


# The files of one atlas, by their index in the group: `files` their bytes (None for a path not read
# as bytes), `probed` their (h, w, kind), `host` {index: BGR array} the images already read on the
# host, `stored` {index: the store's (chunk, byte offset, h, w)}, (hm, wm) the atlas size.
_Group = collections.namedtuple('_Group', 'files probed host stored hm wm')


def _next_group(paths, at, store, decoder):
    """The next group of files from paths[at:] -> _Group, never empty.  A path the store holds is not
    opened: it is in `stored` and its size is the store's.  Any other path goes the way `decoder`
    says.  'device': read and probed; a file the device does not decode, or one with a side above
    DECODE_MAX_SIDE, is read with _imread into `host` as well.  'host': read with _imread into
    `host` only.  A group ends at DECODE_GROUP files or before the file that would take the atlas
    past DECODE_ATLAS_BYTES; a file with a side above DECODE_MAX_SIDE is a group of its own."""
    files, probed, host, stored, hm, wm = [], [], {}, {}, 1, 1
    while at + len(files) < len(paths) and len(files) < DECODE_GROUP:
        i = len(files)
        ent = store.get(paths[at + i]) if store is not None else None
        data = img = None
        if ent is not None:
            h, w, kind = ent[2], ent[3], 0
        elif decoder == 'device':
            with open(paths[at + i], 'rb') as f:
                data = f.read()
            h, w, kind = utils.jpeg_probe(data)
            if kind != 0 or max(h, w) > DECODE_MAX_SIDE:
                img = _imread(paths[at + i])  # (fails here as it fails on the host path)
                h, w = img.shape[:2]
        else:
            img = _imread(paths[at + i])
            h, w, kind = img.shape[0], img.shape[1], 1
        big = max(h, w) > DECODE_MAX_SIDE
        if files and (big or (i + 1) * max(hm, h) * max(wm, w) * 3 > DECODE_ATLAS_BYTES):
            break  # this file starts the next group (nothing of it is kept here)
        if img is not None:
            host[i] = img
        if ent is not None:
            stored[i] = ent
        files.append(data)
        probed.append((h, w, kind))
        hm, wm = max(hm, h), max(wm, w)
        if big:
            break
    return _Group(files, probed, host, stored, hm, wm)


def _group_atlas(group, paths, at, decoder, dev):
    """The atlas of the group at paths[at:] with every slot filled -> (atlas CUDA uint8 [n,H,W,3],
    sizes int32 [n,2] (h, w)).  One host-read file (an oversize one): its pixels are the atlas.
    Stored faces, or files `decoder` = 'host' read: one utils.faces_to_atlas launch makes the atlas
    and fills the stored faces' slots; the files that are neither are decoded by one
    utils.jpeg_decode call and copied slot by slot.  Otherwise one utils.jpeg_decode call over all
    files makes the atlas.  The host-read images go into their slots last; a file whose scan turns
    out to be damaged is read with _imread then and joins `group.host`, which is updated in place."""
    files, probed, host, stored = group.files, group.probed, group.host, group.stored
    n = len(files)
    if n == 1 and host:
        atlas = torch.from_numpy(np.ascontiguousarray(host[0])[None]).to(dev)
        return atlas, np.array([host[0].shape[:2]], np.int32)
    if stored or decoder != 'device':
        sizes, status = np.array([p[:2] for p in probed], np.int32).reshape(-1, 2), np.zeros(n, np.int32)
        faces = [None] * n
        for i, (chunk, off, h, w) in stored.items():
            faces[i] = chunk[off:off + h * w * 3]
        atlas = utils.faces_to_atlas(faces, sizes, group.hm, group.wm, dev)
        rest = [i for i in range(n) if i not in stored and i not in host]
        if rest:
            sub, ssz, sst = utils.jpeg_decode([files[i] for i in rest], dev, probed=[probed[i] for i in rest])
            for j, i in enumerate(rest):
                status[i] = sst[j]
                if sst[j] == 0:
                    h, w = int(ssz[j, 0]), int(ssz[j, 1])
                    atlas[i, :h, :w] = sub[j, :h, :w]
    else:
        atlas, sizes, status = utils.jpeg_decode(files, dev, probed=probed, min_size=(group.hm, group.wm))
    for i in np.flatnonzero(status != 0).tolist():
        if i not in host:  # the scan turned out to be damaged
            host[i] = _imread(paths[at + i])
    for i, img in host.items():
        h, w = img.shape[:2]
        if h > atlas.shape[1] or w > atlas.shape[2]:  # (a reader that disagrees with the frame header)
            grown = torch.zeros((n, max(h, atlas.shape[1]), max(w, atlas.shape[2]), 3),
                                dtype=torch.uint8, device=dev)
            grown[:, :atlas.shape[1], :atlas.shape[2]] = atlas
            atlas = grown
        atlas[i, :h, :w] = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
        sizes[i] = (h, w)
    return atlas, sizes


def _encode_faces_device(paths, model, bs, area, store, decoder):
    """encode_faces with the faces' pixels gathered in HBM, in groups that share an atlas
    (_next_group, _group_atlas), whatever `bs` is: taken from `store` (a facestore.FaceStore or
    None) where it holds the path, else decoded on the GPU (decoder='device'; a file the device does
    not decode is read with _imread) or read with _imread ('host').  Every group's blobs come from
    the blob kernel model(images) runs, and the forward runs on the same batches of `bs` blobs in
    the same order, so the embeddings are the host path's bits."""
    dev = nat.device_of(model)
    x, pending = [], None  # blobs that wait for a full batch

    def flush(blobs, last):
        nonlocal pending
        pending = blobs if pending is None else torch.cat([pending, blobs])
        while pending.shape[0] >= bs or (last and pending.shape[0]):
            x.append(model.encode_blob(pending[:bs]))
            pending = pending[bs:]

    at = 0
    while at < len(paths):
        group = _next_group(paths, at, store, decoder)
        atlas, sizes = _group_atlas(group, paths, at, decoder, dev)
        crops = utils.slot_rects(sizes)
        if area:
            crops[:, 1:] = [_area_rect(int(h), int(w), area) for h, w in sizes]
        at += len(group.files)
        flush(model.blob_from_frames(atlas, crops), at >= len(paths))
    return np.concatenate(x)


def encode_faces(paths, model, bs, area, jpeg_decoder='host', store=None):
    """grouping.py:29-40: batches of images -> model -> concatenated [N, D].  jpeg_decoder='device'
    (an addition) decodes the files on the GPU instead of one by one on the host: the same pixels,
    the same blob kernel and forward, the same embeddings.  store (an addition, a
    facestore.FaceStore the detection stage filled): the faces it holds are taken from HBM and their
    files are not opened; the rest go the way jpeg_decoder says.  The same embeddings again."""
    from .facestore import FaceStore
    if jpeg_decoder not in ('host', 'device'):
        raise ValueError("jpeg_decoder must be 'host' or 'device'")
    if store is not None and not isinstance(store, FaceStore):
        raise ValueError('store must be a FaceStore or None')
    print('Extracting features from images for grouping')
    if len(paths) and (store is not None or jpeg_decoder == 'device'):
        return _encode_faces_device(paths, model, bs, area, store, jpeg_decoder)
    x = []
    for bn in range(math.ceil(len(paths) / bs)):
        images = [_imread(p) for p in paths[bs * bn:bs * (bn + 1)]]
        if area:
            images = [utils.crop_to_area(img, area) for img in images]
        x.append(model(images))
    return np.concatenate(x)


def cosine_classify_device(X, R, device=None):
    """classify's distances (grouping.py:51-55): min / first argmin over the reference rows of
    sklearn's cosine_distances(X, R), in sklearn's bits, on `device` (default cuda:0)."""
    dev = nat.require_gpu(device)
    Xd = torch.from_numpy(np.ascontiguousarray(X, np.float32)).to(dev)
    Rd = torch.from_numpy(np.ascontiguousarray(R, np.float32)).to(dev)
    n, d = Xd.shape
    mins = torch.empty(n, dtype=torch.float32, device=dev)
    inds = torch.empty(n, dtype=torch.int64, device=dev)
    nat.check(nat.lib().vtf_cosine_classify(nat.ptr(Xd), n, nat.ptr(Rd), Rd.shape[0], d, nat.ptr(mins), nat.ptr(inds),
                                            nat.stream_ptr(dev)))
    return mins.cpu().numpy(), inds.cpu().numpy()


def cosine_distances_device(X, R, device=None):
    """sklearn.metrics.pairwise.cosine_distances(X, R) (grouping.py:51) in sklearn's bits, [N, C]."""
    dev = nat.require_gpu(device)
    Xd = torch.from_numpy(np.ascontiguousarray(X, np.float32)).to(dev)
    Rd = torch.from_numpy(np.ascontiguousarray(R, np.float32)).to(dev)
    n, d = Xd.shape
    dist = torch.empty((n, Rd.shape[0]), dtype=torch.float32, device=dev)
    nat.check(nat.lib().vtf_cosine_distances_xr(nat.ptr(Xd), n, nat.ptr(Rd), Rd.shape[0], d, nat.ptr(dist),
                                                nat.stream_ptr(dev)))
    return dist.cpu().numpy()


def classify(X, R, classes, thr, log, paths, out_dir, device=None):
    mins, inds = cosine_classify_device(X, R, device)
    if thr and thr != -1:
        inds[mins >= thr] = len(classes)
        classes.append('other')
    if log:
        dist = cosine_distances_device(X, R, device)  # the same bits as the reference's dist
        fnames = [osp.basename(p) for p in paths]
        with open(osp.join(out_dir, 'faces', 'log_classification.csv'), 'w') as f:
            extra = '(other_threshold=%s)' % str(thr) if thr else ''
            f.write('file_name,' + ','.join(['dist_' + c for c in classes if c != 'other']) +
                    ',assigned_to_class' + extra + '\n')
            for i in range(X.shape[0]):
                f.write('%s,' % fnames[i] + ','.join(['%.4f' % d for d in dist[i]]) + ',%s\n' % classes[inds[i]])
    return inds, classes


def cluster_sweep(X, clusters, random_state, grouper=None, device=None, sharded=False, replicated=False):
    """KMeans + (silhouette, CH, DB) for every k in `clusters`, in order -- cluster_faces'
    loops (grouping.py:97-107).  sharded=True (a collective over the default process group:
    every rank passes the same X, which is checked) splits the work across the ranks
     with no cross-rank reduction inside a result, so every number equals the
    one-process result; the results travel by tensor all-gathers (RCCL on GPUs):
      * KMeans fits by k: rank r fits the k at positions i % world == r; labels all-gathered;
      * silhouette by rows: one pass over the distance rows of the rank's row range computes
        silhouette_samples for EVERY k at once (no N x N matrix anywhere); the per-row values
        are all-gathered and averaged in row order as silhouette_score's np.mean does;
      * CH / DB by k, like the fits.
    `grouper` defaults to the device Grouper (videotofaces.kmeans); tests pass a CPU stand-in.
    replicated=True: the caller has already checked that every rank holds X (no digest here)."""
    import torch
    import torch.distributed as dist
    if grouper is None:
        from .kmeans import Grouper
        grouper = Grouper(device)
    g = grouper
    X = np.ascontiguousarray(X, np.float32)
    world = dist.get_world_size() if sharded and dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    if world > 1:
        from .parallel import all_gather_cpu, all_gather_slots, check_replicated
        if not replicated:
            check_replicated(X, 'cluster_sweep')
    prep = g.prepare(X)
    K, n = len(clusters), X.shape[0]
    idx = [i for i in range(K) if i % world == rank]
    fits = {i: np.asarray(g.kmeans(X, clusters[i], random_state=random_state, prep=prep)) for i in idx}
    if world > 1:
        fits = dict(enumerate(all_gather_slots(fits, K, (n,), torch.int64)))
    labels = [fits[i] for i in range(K)]
    lo, hi = n * rank // world, n * (rank + 1) // world
    sil = g.silhouette_sweep(X, labels, lo, hi) if labels else np.zeros((0, 0), np.float32)
    chdb = {i: (g.calinski_harabasz_score(X, labels[i]), g.davies_bouldin_score(X, labels[i])) for i in idx}
    if world > 1:
        if K:  # row-major [rows, K] blocks in rank order -> [K, n]
            sil = all_gather_cpu(torch.from_numpy(np.ascontiguousarray(np.asarray(sil, np.float32).T))).numpy().T
        chdb = dict(enumerate(tuple(float(v) for v in a)
                              for a in all_gather_slots(chdb, K, (2,), torch.float64)))
    scores = [(clusters[i], float(np.mean(sil[i])), float(chdb[i][0]), float(chdb[i][1]))
              for i in range(len(clusters))]
    return labels, scores


def cluster_faces(paths, X, cluster_params, device=None):
    """grouping.py:92-137 with the KMeans / score sweep on the GPU (cluster_sweep); `device`
    (an addition) picks the GPU."""
    clusters, save_all, rstate, log, out_dir = cluster_params
    clusters = [c for c in clusters if c <= len(paths)]
    print('Clustering images into %s groups' % ', '.join([str(cl) for cl in clusters]))
    labels, scores = cluster_sweep(X, clusters, rstate, device=device)
    if log:
        with open(osp.join(out_dir, 'faces', 'log_clustering.csv'), 'w') as f:
            f.write('n_clusters,silhouette_score,calinski_harabasz_score,davies_bouldin_score\n')
            for score in scores:
                f.write('%u,%s,%s,%s\n' % score)
    if not save_all:
        best_k = max(scores, key=lambda x: x[1])[0]
        i = clusters.index(best_k)
        clusters, labels = [clusters[i]], [labels[i]]
        print('The number of groups chosen: %u' % best_k)
    print('Grouped %u images into %s folders:' % (len(paths), '/'.join([str(cl) for cl in clusters])))
    img_dir = osp.dirname(osp.abspath(paths[0]))
    for i in range(len(clusters)):
        k = clusters[i]
        sub = 'G%u' % k if len(clusters) > 1 else ''
        for j in range(k):
            os.makedirs(osp.join(img_dir, sub, str(j)), exist_ok=True)
        for j in range(len(paths)):
            shutil.copyfile(paths[j], osp.join(img_dir, sub, str(labels[i][j]), osp.basename(paths[j])))
        values, counts = np.unique(labels[i], return_counts=True)
        print((sub + ': ' if sub else '') + ', '.join(['%u: %u' % (v, c) for v, c in zip(values, counts)]))
    print()
    for p in paths:
        os.remove(p)
    return clusters, labels, scores


def encode_refs(refs, model):
    """grouping.py:43-47: the first image of every reference class."""
    return model([_imread(ps[0]) for (_, ps) in refs])


def classify_faces(paths, X, model, classif_params, device=None):
    """grouping.py:69-89: classify against reference images, move files into class folders."""
    refs, thr, log, out_dir = classif_params
    classes = [c for (c, _) in refs]
    print('Found %u classes in ref_dir: %s' % (len(classes), ', '.join(classes)))
    print('Extracting features from reference images')
    R = encode_refs(refs, model)
    print('Classifying images')
    inds, classes = classify(X, R, classes, thr, log, paths, out_dir, device or nat.device_of(model))
    img_dir = osp.dirname(osp.abspath(paths[0]))
    for c in classes:
        os.makedirs(osp.join(img_dir, c), exist_ok=True)
    for p, i in zip(paths, inds):
        os.replace(p, osp.join(img_dir, classes[i], osp.basename(p)))
    print('Grouped %u images into %u folders:' % (len(paths), len(classes)))
    for i, c in enumerate(classes):
        print('%s: %u' % (c, np.count_nonzero(inds == i)))
    print()
    return inds, classes
