"""Detect/describe every image, then match every requested pair — batched on the MI355X.

Drop-in for gtsfm/frontend/correspondence_generator/det_desc_correspondence_generator.py:17-87
(DetDescCorrespondenceGenerator). Same constructor (matcher, detector_descriptor), same
`generate_correspondences(client, images, image_pairs)` signature and outputs: the keypoints of every image and a
dict (i1, i2) -> (M, 2) uint32 putative correspondences (np.array([]) for a pair without matches,
twoway_matcher.py:71-72,80-81).

The reference submits one Dask task per image and one per pair (:64-80). Here the HIP plugin combinations of the
BASELINE configs run batched on the device: images of one size go through ONE batched extraction launch sequence
(per workspace-bounded group), their features stay in HBM as one padded (n, k, D) block, and the pairs go through one
batched matcher launch per chunk of pairs:
- SIFTDetectorDescriptor + TwoWayMatcher (configs C1, C2, C4): the exact-integer fp16 MFMA distance GEMM;
- SuperPointDetectorDescriptor + TwoWayMatcher (config C3): the F16_RERANK matcher on the float descriptors;
- SuperPointDetectorDescriptor + SuperGlueMatcher (config C5): batched SuperGlue (superglue.hip);
- D2NetDetDesc + TwoWayMatcher (the reference's d2net.yaml): the F16_RERANK matcher on the 512-D descriptors.
The reference's shipped configs wrap both plugins in caches (sift_front_end.yaml:23-33: DetectorDescriptorCacher
around SIFT, MatcherCacher around TwoWayMatcher). Those wrappers are looked through: every image and pair is first
answered from the cache directory under the reference's keys (detector_descriptor_cacher.py:58-69,
matcher_cacher.py:82-192), and only the misses go through the batched launches above; their results are written back
under the same keys and payloads, exactly what the per-call cachers would have written. Any other combination runs
its own per-call methods in the reference's order.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from gtsfm_amd import device, native
from gtsfm_amd.common import upload
from gtsfm_amd.common.image import Image
from gtsfm_amd.common.keypoints import Keypoints
from gtsfm_amd.frontend.cacher.detector_descriptor_cacher import DetectorDescriptorCacher
from gtsfm_amd.frontend.cacher.matcher_cacher import MatcherCacher
from gtsfm_amd.frontend.correspondence_generator.correspondence_generator_base import CorrespondenceGeneratorBase
from gtsfm_amd.frontend.detector_descriptor.d2net import D2NetDetDesc, resized_shape
from gtsfm_amd.frontend.detector_descriptor.detector_descriptor_base import DetectorDescriptorBase
from gtsfm_amd.frontend.detector_descriptor.sift import SIFTDetectorDescriptor, extract_group, sift_groups
from gtsfm_amd.frontend.matcher.matcher_base import MatcherBase
from gtsfm_amd.frontend.detector_descriptor.superpoint import SuperPointDetectorDescriptor
from gtsfm_amd.frontend.matcher.lightglue_matcher import LightGlueMatcher
from gtsfm_amd.frontend.matcher.superglue_matcher import MATCH_THRESHOLD, SuperGlueMatcher
from gtsfm_amd.frontend.matcher.twoway_matcher import MatchingDistanceType, TwoWayMatcher
import gtsfm_amd.utils.io as io_utils

PAIR_CHUNK = 8192  # pairs per matcher launch: (chunk, k, 2) int32 indices = 128 MiB at k = 2048


def resolve(obj):
    """Images may arrive as Dask futures (the reference's call site) or as plain objects."""
    return obj.result() if hasattr(obj, "result") and callable(obj.result) else obj


class DeviceFeatures:
    """Features of n images resident in HBM: xy (n, k, 2) f32, desc (n, k, D) f32, count (n,) int32."""

    def __init__(self, xy: torch.Tensor, desc: torch.Tensor, count: torch.Tensor, keypoints: List[Keypoints]):
        self.xy, self.desc, self.count, self.keypoints = xy, desc, count, keypoints


def extract_sift_batched(detector: SIFTDetectorDescriptor, images: Sequence[Image]) -> DeviceFeatures:
    """gtsfm_sift_batched launch sequences per image size (workspace-bounded groups); features gathered into one
    padded block."""
    dev = upload.cuda_device()
    n, k = len(images), detector.max_keypoints
    xy = torch.zeros((n, k, 2), dtype=torch.float32, device=dev)
    attr = torch.zeros((n, k, 3), dtype=torch.float32, device=dev)
    desc = torch.zeros((n, k, 128), dtype=torch.float32, device=dev)
    count = torch.zeros((n,), dtype=torch.int32, device=dev)
    for idx in sift_groups(list(images), k):  # same shape, workspace-bounded; masks as detectAndCompute's
        res = extract_group(list(images), idx, k)
        sel = torch.tensor(idx, dtype=torch.long, device=dev)
        xy[sel], attr[sel], desc[sel], count[sel] = res.xy, res.attr, res.desc, res.count
    cnt = count.cpu().numpy()
    xy_h, attr_h = xy.cpu().numpy(), attr.cpu().numpy()
    kps = [Keypoints(coordinates=xy_h[i, : cnt[i]].astype(np.float64), scales=attr_h[i, : cnt[i], 0].astype(np.float64),
                     responses=attr_h[i, : cnt[i], 2].astype(np.float64)) for i in range(n)]
    return DeviceFeatures(xy, desc, count, kps)


def match_pairs_batched(feats: DeviceFeatures, image_pairs: Sequence[Tuple[int, int]], ratio, mode: int,
                        chunk: int = PAIR_CHUNK) -> Dict[Tuple[int, int], np.ndarray]:
    """All pairs through gtsfm_match_batched, `chunk` pairs per launch; host dict in the reference's format."""
    out: Dict[Tuple[int, int], np.ndarray] = {}
    pairs = np.asarray(image_pairs, dtype=np.int64).reshape(-1, 2)
    dev = feats.desc.device
    G = device.match_group_size(feats.desc.shape[1], feats.desc.shape[2]) if mode == native.GTSFM_MATCH_INT_F16 else 0
    for s in range(0, len(pairs), chunk):
        blk = pairs[s: s + chunk]
        groups = torch.from_numpy(device.pair_groups(blk, G)).to(dev) if G > 1 else None
        idx, cnt = device.match_pairs(feats.desc, feats.count, torch.from_numpy(blk.astype(np.int32)).to(dev),
                                      ratio, mode, groups=groups)
        cnt_h = cnt.cpu().numpy()
        width = int(cnt_h.max()) if len(cnt_h) else 0
        idx_h = idx[:, :width].cpu().numpy().view(np.uint32)
        for j, (i1, i2) in enumerate(blk):
            m = int(cnt_h[j])
            out[(int(i1), int(i2))] = idx_h[j, :m].copy() if m else np.array([])
    return out


SP_GROUP_BYTES = 16 << 30  # SuperPoint workspace per launch (~0.75 GB per 1080p image)


def extract_superpoint_batched(detector: SuperPointDetectorDescriptor, images: Sequence[Image]) -> DeviceFeatures:
    """gtsfm_superpoint_batched per image size in workspace-bounded groups; features gathered into one padded block
    (scores kept for SuperGlue). Image masks filter the detections on the device before the top-k, as the per-call
    plugin (reference superpoint.py:68-72)."""
    dev = upload.cuda_device()
    n, k = len(images), detector.max_keypoints
    xy = torch.zeros((n, k, 2), dtype=torch.float32, device=dev)
    sc = torch.zeros((n, k), dtype=torch.float32, device=dev)
    desc = torch.zeros((n, k, 256), dtype=torch.float32, device=dev)
    count = torch.zeros((n,), dtype=torch.int32, device=dev)
    by_shape: Dict[tuple, List[int]] = {}
    for i, im in enumerate(images):
        by_shape.setdefault(tuple(im.value_array.shape), []).append(i)
    L = native.lib()
    for shape, idx in by_shape.items():
        per = max(1, int(L.gtsfm_superpoint_workspace_bytes(1, shape[0], shape[1], k)))
        g = max(1, SP_GROUP_BYTES // per)
        for s0 in range(0, len(idx), g):
            part = idx[s0: s0 + g]
            res = detector.extract_batch([images[i].value_array for i in part], k, masks=[images[i].mask for i in part])
            sel = torch.tensor(part, dtype=torch.long, device=dev)
            xy[sel], sc[sel], desc[sel], count[sel] = res.xy, res.scores, res.desc, res.count
    cnt = count.cpu().numpy()
    xy_h, sc_h = xy.cpu().numpy(), sc.cpu().numpy()
    kps = [Keypoints(coordinates=xy_h[i, : cnt[i]], scales=None, responses=sc_h[i, : cnt[i]]) for i in range(n)]
    out = DeviceFeatures(xy, desc, count, kps)
    out.scores = sc
    return out


D2NET_GROUP_BYTES = 16 << 30  # D2-Net workspace per launch


def extract_d2net_batched(detector: D2NetDetDesc, images: Sequence[Image]) -> DeviceFeatures:
    """gtsfm_d2net_batched per image size in workspace-bounded groups; features gathered into one padded block
    (descending score order per image, scores kept as the keypoints' responses, as D2NetDetDesc._unpack)."""
    dev = upload.cuda_device()
    n, k = len(images), detector.max_keypoints
    xy = torch.zeros((n, k, 2), dtype=torch.float32, device=dev)
    sc = torch.zeros((n, k), dtype=torch.float32, device=dev)
    desc = torch.zeros((n, k, 512), dtype=torch.float32, device=dev)
    count = torch.zeros((n,), dtype=torch.int32, device=dev)
    by_shape: Dict[tuple, List[int]] = {}
    for i, im in enumerate(images):
        by_shape.setdefault(tuple(im.value_array.shape), []).append(i)
    L = native.lib()
    for shape, idx in by_shape.items():
        h1, w1 = resized_shape(shape[0], shape[1])[:2]  # the network runs on the resized image
        per = max(1, int(L.gtsfm_d2net_workspace_bytes(1, h1, w1, k)))
        g = max(1, D2NET_GROUP_BYTES // per)
        for s0 in range(0, len(idx), g):
            part = idx[s0: s0 + g]
            res = detector.extract_batch([images[i].value_array for i in part], k)
            sel = torch.tensor(part, dtype=torch.long, device=dev)
            xy[sel], sc[sel], desc[sel], count[sel] = res.xy, res.scores, res.desc, res.count
    cnt = count.cpu().numpy()
    xy_h, sc_h = xy.cpu().numpy(), sc.cpu().numpy()
    kps = [Keypoints(coordinates=xy_h[i, : cnt[i]], responses=sc_h[i, : cnt[i]]) for i in range(n)]
    out = DeviceFeatures(xy, desc, count, kps)
    out.scores = sc
    return out


def superglue_pairs_batched(matcher: SuperGlueMatcher, feats: DeviceFeatures, image_shapes: Sequence[tuple],
                            image_pairs: Sequence[Tuple[int, int]], chunk: int = 1024
                            ) -> Dict[Tuple[int, int], np.ndarray]:
    """All pairs through gtsfm_superglue_batched on the resident features, `chunk` pairs per launch sequence (the
    workspace is ~59 MB per pair at 2048 keypoints); host dict in SuperGlueMatcher.match's format."""
    out: Dict[Tuple[int, int], np.ndarray] = {}
    pairs = np.asarray(image_pairs, dtype=np.int64).reshape(-1, 2)
    dev = feats.desc.device
    kmax = feats.desc.shape[1]
    kpad = (kmax + 63) // 64 * 64
    xy, sc, desc = feats.xy, feats.scores, feats.desc
    if kpad != kmax:
        pad = kpad - kmax
        xy = torch.nn.functional.pad(xy, (0, 0, 0, pad))
        sc = torch.nn.functional.pad(sc, (0, pad))
        desc = torch.nn.functional.pad(desc, (0, 0, 0, pad))
    hw = torch.tensor([[int(s[0]), int(s[1])] for s in image_shapes], dtype=torch.int32, device=dev)
    cnt_h = feats.count.cpu().numpy()
    ws = None
    for s in range(0, len(pairs), chunk):
        blk = pairs[s: s + chunk]
        run = blk[(cnt_h[blk[:, 0]] > 0) & (cnt_h[blk[:, 1]] > 0)] if len(blk) else blk
        for i1, i2 in blk:
            out[(int(i1), int(i2))] = np.zeros((0, 2), np.uint32)
        if not len(run):
            continue
        need = int(native.lib().gtsfm_superglue_workspace_bytes(len(run), kpad))
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        idx, c, _ = device.superglue_match(xy.contiguous(), sc.contiguous(), desc.contiguous(), feats.count, hw,
                                           torch.from_numpy(run.astype(np.int32)).to(dev), matcher.weights(),
                                           matcher._n_layers, matcher._config["sinkhorn_iterations"],
                                           MATCH_THRESHOLD, workspace=ws)
        c = c.cpu().numpy()
        w = int(c.max()) if len(c) else 0
        idx_h = idx[:, :w].cpu().numpy().view(np.uint32)
        for j, (i1, i2) in enumerate(run):
            out[(int(i1), int(i2))] = idx_h[j, : c[j]].copy()
    return out


def lightglue_pairs_batched(matcher: LightGlueMatcher, feats: DeviceFeatures, image_shapes: Sequence[tuple],
                            image_pairs: Sequence[Tuple[int, int]], chunk: int = 1024
                            ) -> Dict[Tuple[int, int], np.ndarray]:
    """All pairs through gtsfm_lightglue_batched on the resident features, `chunk` pairs per launch sequence (the
    workspace is ~70 MB per pair at 2048 keypoints); host dict in LightGlueMatcher.match's format."""
    out: Dict[Tuple[int, int], np.ndarray] = {}
    pairs = np.asarray(image_pairs, dtype=np.int64).reshape(-1, 2)
    dev = feats.desc.device
    kmax = feats.desc.shape[1]
    kpad = (kmax + 63) // 64 * 64
    xy, desc = feats.xy, feats.desc
    if kpad != kmax:
        pad = kpad - kmax
        xy = torch.nn.functional.pad(xy, (0, 0, 0, pad))
        desc = torch.nn.functional.pad(desc, (0, 0, 0, pad))
    xy, desc = xy.contiguous(), desc.contiguous()
    hw = torch.tensor([[int(s[0]), int(s[1])] for s in image_shapes], dtype=torch.int32, device=dev)
    cnt_h = feats.count.cpu().numpy()
    ws = None
    for s in range(0, len(pairs), chunk):
        blk = pairs[s: s + chunk]
        run = blk[(cnt_h[blk[:, 0]] > 0) & (cnt_h[blk[:, 1]] > 0)] if len(blk) else blk
        for i1, i2 in blk:
            out[(int(i1), int(i2))] = np.zeros((0, 2), np.uint32)
        if not len(run):
            continue
        need = int(native.lib().gtsfm_lightglue_workspace_bytes(len(run), kpad))
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        idx, c, _, _ = device.lightglue_match(xy, desc, feats.count, hw, torch.from_numpy(run.astype(np.int32)).to(dev),
                                              matcher.weights(), matcher._n_layers, matcher._depth_confidence,
                                              matcher._filter_threshold, workspace=ws)
        c = c.cpu().numpy()
        w = int(c.max()) if len(c) else 0
        idx_h = idx[:, :w].cpu().numpy().view(np.uint32)
        for j, (i1, i2) in enumerate(run):
            out[(int(i1), int(i2))] = idx_h[j, : c[j]].copy()
    return out


def features_from_host(entries: Sequence[Tuple[Keypoints, np.ndarray]], kmin: int, dim: int,
                       with_scores: bool) -> DeviceFeatures:
    """Host (keypoints, descriptors) per image -> one padded device block (cache hits enter the batched path here)."""
    n = len(entries)
    k = max([kmin] + [len(kp) for kp, _ in entries])
    xy = np.zeros((n, k, 2), np.float32)
    desc = np.zeros((n, k, dim), np.float32)
    sc = np.zeros((n, k), np.float32)
    count = np.zeros((n,), np.int32)
    for i, (kp, d) in enumerate(entries):
        m = len(kp)
        d = np.asarray(d).reshape(m, -1) if m else np.zeros((0, dim), np.float32)
        if m and d.shape[1] != dim:
            raise ValueError(f"cached descriptors have {d.shape[1]} dims, the detector gives {dim}")
        count[i] = m
        xy[i, :m] = kp.coordinates
        desc[i, :m] = d
        if with_scores and kp.responses is not None:
            sc[i, :m] = kp.responses
    dev = torch.device("cuda")
    out = DeviceFeatures(torch.from_numpy(xy).to(dev), torch.from_numpy(desc).to(dev), torch.from_numpy(count).to(dev),
                         [kp for kp, _ in entries])
    if with_scores:
        out.scores = torch.from_numpy(sc).to(dev)
    return out


def merge_features(parts: Sequence[Tuple[List[int], DeviceFeatures]], n: int) -> DeviceFeatures:
    """Scatters per-subset device blocks (e.g. cache hits and batched misses) into one block over all n images."""
    k = max(f.desc.shape[1] for _, f in parts)
    dim = parts[0][1].desc.shape[2]
    dev = parts[0][1].desc.device
    with_scores = all(hasattr(f, "scores") for _, f in parts)
    xy = torch.zeros((n, k, 2), dtype=torch.float32, device=dev)
    desc = torch.zeros((n, k, dim), dtype=torch.float32, device=dev)
    count = torch.zeros((n,), dtype=torch.int32, device=dev)
    sc = torch.zeros((n, k), dtype=torch.float32, device=dev) if with_scores else None
    kps: List[Optional[Keypoints]] = [None] * n
    for idx, f in parts:
        if not idx:
            continue
        sel = torch.tensor(idx, dtype=torch.long, device=dev)
        kk = f.desc.shape[1]
        xy[sel, :kk], desc[sel, :kk], count[sel] = f.xy, f.desc, f.count
        if sc is not None:
            sc[sel, :kk] = f.scores
        for j, i in enumerate(idx):
            kps[i] = f.keypoints[j]
    out = DeviceFeatures(xy, desc, count, kps)  # type: ignore[arg-type]
    if sc is not None:
        out.scores = sc
    return out


class DetDescCorrespondenceGenerator(CorrespondenceGeneratorBase):
    """Traditional detect -> describe -> match, batched on the device when the plugins are the HIP ones."""

    def __init__(self, matcher: MatcherBase, detector_descriptor: DetectorDescriptorBase) -> None:
        self._detector_descriptor = detector_descriptor
        self._matcher = matcher
        self.device_features: DeviceFeatures | None = None  # last batched extraction (kept for reuse)

    def __repr__(self) -> str:
        return f"DetDescCorrespondenceGenerator:\n   {self._detector_descriptor}\n   {self._matcher}\n"

    def _plugins(self):
        """(detector, detector cache or None, matcher, matcher cache or None): the reference configs' cachers are
        looked through so that the plugins they wrap can run batched."""
        d, m = self._detector_descriptor, self._matcher
        dc = d if type(d) is DetectorDescriptorCacher else None
        mc = m if type(m) is MatcherCacher else None
        return (dc.wrapped if dc else d), dc, (mc.wrapped if mc else m), mc

    def _batched(self) -> Optional[str]:
        """Which batched device path serves this plugin pair: 'sift', 'superpoint_twoway', 'superpoint_superglue',
        'superpoint_lightglue', 'd2net_twoway', or None (per-call)."""
        d, _, m, _ = self._plugins()
        twoway_l2 = type(m) is TwoWayMatcher and m._distance_type is MatchingDistanceType.EUCLIDEAN
        if type(d) is SIFTDetectorDescriptor and twoway_l2:
            return "sift"
        if type(d) is SuperPointDetectorDescriptor and twoway_l2:
            return "superpoint_twoway"
        if type(d) is SuperPointDetectorDescriptor and type(m) is SuperGlueMatcher:
            return "superpoint_superglue"
        if type(d) is SuperPointDetectorDescriptor and type(m) is LightGlueMatcher:
            return "superpoint_lightglue"
        if type(d) is D2NetDetDesc and twoway_l2:
            return "d2net_twoway"
        return None

    @staticmethod
    def _extractor(path: str):
        """(batched extraction, descriptor width) of a path; the module's functions as they are at call time."""
        if path == "sift":
            return extract_sift_batched, 128
        if path == "d2net_twoway":
            return extract_d2net_batched, 512
        return extract_superpoint_batched, 256

    def _extract(self, path: str, imgs: List[Image]) -> Tuple[DeviceFeatures, List[np.ndarray]]:
        """Batched extraction of every image that the detector cache (if any) does not hold; the first 10
        descriptor rows of every image as the per-call path would hand them to the matcher cache's key."""
        d, dc, _, _ = self._plugins()
        extract, dim = self._extractor(path)
        if dc is None:
            return extract(d, imgs), None
        hit_idx, hit_entries, miss = [], [], []
        for i, im in enumerate(imgs):
            c = dc.cache_lookup(im)
            if c is None:
                miss.append(i)
            else:
                hit_idx.append(i)
                hit_entries.append(c)
        heads: List[np.ndarray] = [None] * len(imgs)  # type: ignore[list-item]
        parts: List[Tuple[List[int], DeviceFeatures]] = []
        if miss:
            fm = extract(d, [imgs[i] for i in miss])
            cnt = fm.count.cpu().numpy()
            desc_h = fm.desc.cpu().numpy()
            for j, i in enumerate(miss):
                dj = desc_h[j, : cnt[j]].copy()  # exactly the per-call plugin's descriptors
                dc.cache_store(imgs[i], fm.keypoints[j], dj)
                heads[i] = dj[:10]
            parts.append((miss, fm))
        if hit_entries:
            parts.append((hit_idx, features_from_host(hit_entries, d.max_keypoints, dim,
                                                      with_scores=path != "sift")))
            for i, (_, dsc) in zip(hit_idx, hit_entries):
                heads[i] = np.asarray(dsc)[:10]
        if not hit_entries:
            return parts[0][1], heads
        feats = merge_features(parts, len(imgs))
        feats.from_host = True
        return feats, heads

    def _match(self, path: str, feats: DeviceFeatures, imgs: List[Image], image_pairs: Sequence[Tuple[int, int]],
               heads: Optional[List[np.ndarray]]) -> Dict[Tuple[int, int], np.ndarray]:
        """Batched matching of every pair that the matcher cache (if any) does not hold; misses written back."""
        _, _, m, mc = self._plugins()
        if mc is not None and heads is None:
            head = feats.desc[:, :10].cpu().numpy()
            cnt = feats.count.cpu().numpy()
            heads = [head[i, : min(10, cnt[i])] for i in range(len(imgs))]
        pairs = [(int(a), int(b)) for a, b in image_pairs]
        corr: Dict[Tuple[int, int], np.ndarray] = {}
        paths = {}
        todo = pairs
        if mc is not None:
            todo = []
            for (i1, i2) in pairs:
                p = mc.cache_path(feats.keypoints[i1], feats.keypoints[i2], heads[i1], heads[i2], imgs[i1].shape,
                                  imgs[i2].shape)
                c = io_utils.read_from_bz2_file(p)
                if c is None:
                    todo.append((i1, i2))
                    paths[(i1, i2)] = p
                else:
                    corr[(i1, i2)] = c
        if todo:
            if path == "superpoint_superglue":
                got = superglue_pairs_batched(m, feats, [im.value_array.shape for im in imgs], todo)
            elif path == "superpoint_lightglue":
                got = lightglue_pairs_batched(m, feats, [im.value_array.shape for im in imgs], todo)
            else:
                got = match_pairs_batched(feats, todo, m._ratio_test_threshold, self._match_mode(path, feats))
            for key in todo:
                if mc is not None:
                    io_utils.write_to_bz2_file(got[key], paths[key])
                corr[key] = got[key]
        return {key: corr[key] for key in pairs}

    @staticmethod
    def _match_mode(path: str, feats: DeviceFeatures) -> int:
        if path != "sift":
            # float descriptors (SuperPoint 256-D, D2-Net 512-D, both within GTSFM_MATCH_F16_MAX_DIM): fp16 MFMA
            # shortlist + certified exact re-rank (same matches as EXACT_F32)
            return native.GTSFM_MATCH_F16_RERANK
        if getattr(feats, "from_host", False):
            # cache entries (e.g. OpenCV's descriptors written by the reference) are checked, not assumed, to be the
            # small integers the exact fp16 path needs (TwoWayMatcher.select_match_mode's test); every mode gives
            # the same matches, so one mode for the whole block is only a speed choice
            d = feats.desc
            ok = (d.shape[2] <= 139 and d.shape[1] <= 8192 and bool((d >= 0).all()) and bool((d <= 1023).all())
                  and bool((d == torch.round(d)).all())
                  and bool(((d.double() ** 2).sum(-1) < float(1 << 19)).all()))
            return native.GTSFM_MATCH_INT_F16 if ok else native.GTSFM_MATCH_F16_RERANK
        # HIP SIFT descriptors are integers in [0, 255] with |d|^2 < 2^19: the exact fp16 MFMA path applies
        return native.GTSFM_MATCH_INT_F16

    def generate_correspondences(
        self, client, images: List, image_pairs: List[Tuple[int, int]]
    ) -> Tuple[List[Keypoints], Dict[Tuple[int, int], np.ndarray]]:
        imgs = [resolve(im) for im in images]
        path = self._batched()
        if path is not None:
            feats, heads = self._extract(path, imgs)
            self.device_features = feats
            return feats.keypoints, self._match(path, feats, imgs, image_pairs, heads)
        features = [self._detector_descriptor.detect_and_describe(im) for im in imgs]
        corr = {}
        for (i1, i2) in image_pairs:
            corr[(i1, i2)] = self._matcher.match(features[i1][0], features[i2][0], features[i1][1],
                                                 features[i2][1], imgs[i1].shape, imgs[i2].shape)
        return [f[0] for f in features], corr
