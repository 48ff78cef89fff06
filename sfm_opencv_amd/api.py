"""Python binding of the C-ABI (include/sfmhip.h) + a mirror of the reference's hot-path functions.

Names and argument meaning follow OpenCV_SFM/NViewReconstuct.cpp: match_features (873), match_features_for_all (850),
get_matched_points (989), reconstruct (1117), bundle_adjustment (1162).  cv::Mat / std::vector arguments become numpy
arrays (host entry points) or torch CUDA tensors (device entry points); outputs are returned instead of filled.
Everything here calls libsfmhip.so; nothing falls back to the CPU.
"""
import collections
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import BAOptions, BASummary, SfmHipError

DMATCH = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])


def _ptr(a):
    """address of a numpy array or a torch tensor"""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()


def _dptr(a):
    """a device address for the C-ABI: None / 0 -> NULL, an integer as it is, else a torch tensor's data_ptr()"""
    if a is None:
        return None
    a = a.data_ptr() if hasattr(a, "data_ptr") else int(a)
    return C.c_void_p(a) if a else None


class DescSet:
    def __init__(self, ctx, handle, rows, keepalive=None):
        self.ctx, self.handle, self.rows, self._keep = ctx, handle, rows, keepalive

    def info(self):
        kind, rows, dim, ex = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self.ctx._check(self.ctx.lib.sfmhip_descset_info(self.handle, kind, rows, dim, ex))
        return dict(kind=kind.value, rows=rows.value, dim=dim.value, exact_u8=bool(ex.value))

    def refresh(self):
        self.ctx._check(self.ctx.lib.sfmhip_descset_refresh(self.handle))

    def close(self):
        if self.handle and self.ctx.h:      # the context owns the stream: never touch a set after its context died
            self.ctx.lib.sfmhip_descset_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One per process / GPU (sfmhip_create)."""

    def __init__(self, device=0, use_torch_stream=False):
        self.lib = _lib.load()
        h = C.c_void_p()
        rc = self.lib.sfmhip_create(int(device), C.byref(h))
        if rc != 0:
            raise SfmHipError(f"sfmhip_create(device={device}) failed with {rc} "
                              "(no usable gfx950 device; there is no CPU fallback)")
        self.h = h
        self.device = device
        self.torch_stream = None
        if use_torch_stream:
            import torch
            st = torch.cuda.current_stream(device)
            if st.cuda_stream == 0:
                # the legacy default stream has handle 0, which the C-ABI reads as "use the context's own stream":
                # make a real stream current so that torch events / copies / collectives and the library share it
                st = torch.cuda.Stream(device=device)
                torch.cuda.set_stream(st)
            self.torch_stream = st
            self.set_stream(st.cuda_stream)

    def _check(self, rc):
        if rc != 0:
            raise SfmHipError(f"libsfmhip error {rc}: {self.lib.sfmhip_last_error(self.h).decode()}")

    def set_stream(self, stream_ptr):
        self._check(self.lib.sfmhip_set_stream(self.h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def synchronize(self):
        self._check(self.lib.sfmhip_synchronize(self.h))

    # ---------------------------------------------------------------- RCCL (multi-GPU)
    def rccl_available(self):
        return bool(self.lib.sfmhip_rccl_available())

    def rccl_unique_id(self):
        """128 opaque bytes from ncclGetUniqueId (rank 0; ship them to the other ranks)"""
        buf = (C.c_char * 128)()
        self._check(self.lib.sfmhip_rccl_get_unique_id(buf))
        return bytes(buf)

    def rccl_comm_create(self, unique_id, rank, world):
        comm = C.c_void_p()
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        self._check(self.lib.sfmhip_rccl_comm_create(self.h, buf, int(rank), int(world), C.byref(comm)))
        return comm

    def rccl_comm_destroy(self, comm):
        self._check(self.lib.sfmhip_rccl_comm_destroy(comm))

    def rccl_allreduce_f64(self, comm, dev_ptr, count):
        self._check(self.lib.sfmhip_rccl_allreduce_f64(self.h, comm, C.c_void_p(int(dev_ptr)), int(count)))

    def trim(self):
        """release the device blocks the context keeps from destroyed BA problems (sfmhip_trim)"""
        self._check(self.lib.sfmhip_trim(self.h))

    def debug_sort_pairs(self, keys, vals=None, bits=64):
        """(keys, values) after the library's stable radix sort of uint64 keys with uint32 values (None: the element index), ordered by
        the low 8 * max(1, ceil(bits / 8)) bits of the keys (sfmhip_debug_sort_pairs, test helper)"""
        k = np.ascontiguousarray(keys, np.uint64)
        v = None if vals is None else np.ascontiguousarray(vals, np.uint32)
        ko = np.empty(k.size, np.uint64); vo = np.empty(k.size, np.uint32)
        self._check(self.lib.sfmhip_debug_sort_pairs(self.h, k.ctypes.data, None if v is None else v.ctypes.data, k.size, int(bits),
                                                     ko.ctypes.data, vo.ctypes.data))
        return ko, vo

    def debug_scan_u32(self, counters):
        """(exclusive prefix sums modulo 2^32 as uint32, the 64-bit total) of uint32 counters (sfmhip_debug_scan_u32, test helper)"""
        a = np.ascontiguousarray(counters, np.uint32)
        out = np.empty(a.size, np.uint32); total = C.c_uint64(0xffffffffffffffff)
        self._check(self.lib.sfmhip_debug_scan_u32(self.h, a.ctypes.data, a.size, out.ctypes.data, C.byref(total)))
        return out, total.value

    def debug_upload_many(self, sources, granules):
        """The uint8 arrays `sources` through the pinned staging ring, back to back with no host wait between them, granule 0 by
        sfm_upload and any other by sfm_upload_produced; returns (what arrived on the device, one uint8 array per source, and
        dict(pieces, bytes, violations, nt) of the produced transfers) (sfmhip_debug_upload_many, test helper)"""
        src = [np.ascontiguousarray(s, np.uint8).reshape(-1) for s in sources]
        n = len(src)
        outs = [np.full(s.size, 0xEE, np.uint8) for s in src]
        ptrs = (C.c_void_p * n)(*[s.ctypes.data for s in src]); optrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        nb = (C.c_size_t * n)(*[s.size for s in src]); gr = (C.c_size_t * n)(*[int(g) for g in granules])
        assert len(granules) == n
        stats = (C.c_uint64 * 4)()
        self._check(self.lib.sfmhip_debug_upload_many(self.h, ptrs, nb, gr, n, optrs, stats))
        return outs, dict(pieces=stats[0], bytes=stats[1], violations=stats[2], nt=stats[3])

    def set_kernel_timing(self, enable=True):
        """bracket every kNN launch sequence with HIP events (sfmhip_set_kernel_timing)"""
        self._check(self.lib.sfmhip_set_kernel_timing(self.h, 1 if enable else 0))

    def match_kernel_ms(self):
        """[kNN kernel ms, merge + re-score ms, calls averaged, 0] since the last query (synchronises)"""
        out = (C.c_double * 4)()
        self._check(self.lib.sfmhip_match_kernel_ms(self.h, out))
        return list(out)

    def close(self):
        if self.h:
            self.lib.sfmhip_destroy(self.h)
            self.h = None

    # ---------------------------------------------------------------- matching
    def descset_l2(self, desc):
        """desc: numpy float32 (rows, dim) on the host, or a torch float32 CUDA tensor (borrowed, must stay alive)."""
        out = C.c_void_p()
        if isinstance(desc, np.ndarray):
            d = np.ascontiguousarray(desc, np.float32)
            rows, dim = d.shape
            self._check(self.lib.sfmhip_descset_create_l2_host(self.h, d.ctypes.data, rows, dim, dim, C.byref(out)))
            return DescSet(self, out, rows)
        assert desc.is_cuda and desc.dim() == 2 and desc.stride(1) == 1
        rows, dim = desc.shape
        self._check(self.lib.sfmhip_descset_create_l2_dev(self.h, desc.data_ptr(), rows, dim, desc.stride(0), C.byref(out)))
        return DescSet(self, out, rows, keepalive=desc)

    def descset_hamming2(self, desc):
        out = C.c_void_p()
        if isinstance(desc, np.ndarray):
            d = np.ascontiguousarray(desc, np.uint8)
            rows, nb = d.shape
            self._check(self.lib.sfmhip_descset_create_hamming2_host(self.h, d.ctypes.data, rows, nb, nb, C.byref(out)))
            return DescSet(self, out, rows)
        assert desc.is_cuda and desc.dim() == 2 and desc.stride(1) == 1
        rows, nb = desc.shape
        self._check(self.lib.sfmhip_descset_create_hamming2_dev(self.h, desc.data_ptr(), rows, nb, desc.stride(0), C.byref(out)))
        return DescSet(self, out, rows, keepalive=desc)

    def descsets_host(self, mats):
        """Many host matrices (float32: L2 / uint8: Hamming2; one row length) in ONE call: sfmhip_descsets_create_{l2,hamming2}_host."""
        if len(mats) == 0:
            return []
        ham = np.asarray(mats[0]).dtype == np.uint8
        dt = np.uint8 if ham else np.float32
        arrs = [np.asarray(m, dt) for m in mats]
        arrs = [a if a.ndim == 2 and a.strides[1] == a.itemsize and a.strides[0] % a.itemsize == 0 and a.strides[0] >= a.shape[1] * a.itemsize
                else np.ascontiguousarray(a) for a in arrs]
        dim = arrs[0].shape[1]
        assert all(a.shape[1] == dim for a in arrs)
        n = len(arrs)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        rows = np.array([a.shape[0] for a in arrs], np.int32)
        # (numpy gives an array without rows the strides (0, 0): its row stride says nothing, and the library wants ld >= dim)
        ld = (C.c_size_t * n)(*[a.strides[0] // a.itemsize if a.shape[0] else dim for a in arrs])
        out = (C.c_void_p * n)()
        fn = self.lib.sfmhip_descsets_create_hamming2_host if ham else self.lib.sfmhip_descsets_create_l2_host
        self._check(fn(self.h, ptrs, rows.ctypes.data, dim, ld, n, out))
        return [DescSet(self, C.c_void_p(out[i]), int(rows[i])) for i in range(n)]

    def refresh_descsets(self, sets):
        """re-run the preparation pass of many sets in one launch (enqueues only)"""
        arr = (C.c_void_p * len(sets))(*[s.handle for s in sets])
        self._check(self.lib.sfmhip_descsets_refresh(self.h, arr, len(sets)))

    def knn2_dev(self, qset, tset, idx2, dist2, force_path=0):
        """idx2 (nq,2) int32 / dist2 (nq,2) float32 torch CUDA tensors; enqueues only."""
        self._check(self.lib.sfmhip_knn2_dev(self.h, qset.handle, tset.handle, idx2.data_ptr(), dist2.data_ptr(), force_path))

    def knn2_mutual_dev(self, qset, tset, idx2, dist2, rev_idx, rev_dist, force_path=0):
        """sfmhip_knn2_mutual_dev: knn2_dev + the nearest query of every train row (rev_idx (nt,) int32 / rev_dist (nt,) float32
        torch CUDA tensors); enqueues only."""
        self._check(self.lib.sfmhip_knn2_mutual_dev(self.h, qset.handle, tset.handle, idx2.data_ptr(), dist2.data_ptr(),
                                                    rev_idx.data_ptr(), rev_dist.data_ptr(), force_path))

    def _knn2_mutual_host(self, sets, nq, nt, force_path):
        import torch
        dev = torch.device("cuda", self.device)
        idx = torch.empty((max(nq, 1), 2), dtype=torch.int32, device=dev); dist = torch.empty((max(nq, 1), 2), dtype=torch.float32, device=dev)
        ridx = torch.empty(max(nt, 1), dtype=torch.int32, device=dev); rdist = torch.empty(max(nt, 1), dtype=torch.float32, device=dev)
        self.knn2_mutual_dev(sets[0], sets[1], idx, dist, ridx, rdist, force_path)
        self.synchronize()
        out = (idx[:nq].cpu().numpy(), dist[:nq].cpu().numpy(), ridx[:nt].cpu().numpy(), rdist[:nt].cpu().numpy())
        for s in sets:
            s.close()
        return out

    def knn2_mutual_l2(self, q, t, force_path=0):
        """(idx2, dist2, rev_idx, rev_dist) of float32 host rows: kNN-2 of q against t and the nearest q row of every t row."""
        q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
        return self._knn2_mutual_host([self.descset_l2(q), self.descset_l2(t)], q.shape[0], t.shape[0], force_path)

    def knn2_mutual_hamming2(self, q, t, force_path=0):
        """the Hamming2 form of knn2_mutual_l2 (uint8 host rows)"""
        q = np.ascontiguousarray(q, np.uint8); t = np.ascontiguousarray(t, np.uint8)
        return self._knn2_mutual_host([self.descset_hamming2(q), self.descset_hamming2(t)], q.shape[0], t.shape[0], force_path)

    def knn2_l2(self, q, t):
        q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
        nq, dim = q.shape; nt = t.shape[0]
        idx = np.empty((nq, 2), np.int32); dist = np.empty((nq, 2), np.float32)
        self._check(self.lib.sfmhip_knn2_l2_f32(self.h, q.ctypes.data, nq, t.ctypes.data, nt, dim, dim, dim,
                                                idx.ctypes.data, dist.ctypes.data))
        return idx, dist

    def knn2_hamming2(self, q, t):
        q = np.ascontiguousarray(q, np.uint8); t = np.ascontiguousarray(t, np.uint8)
        nq, nb = q.shape; nt = t.shape[0]
        idx = np.empty((nq, 2), np.int32); dist = np.empty((nq, 2), np.float32)
        self._check(self.lib.sfmhip_knn2_hamming2_u8(self.h, q.ctypes.data, nq, t.ctypes.data, nt, nb, nb, nb,
                                                     idx.ctypes.data, dist.ctypes.data))
        return idx, dist

    def match_pairs(self, sets, pairs, ratio=0.6, floor_=10.0, mult=5.0, cross_check=False):
        """sets: list of DescSet; pairs: (n_pairs, 2) int.  Returns list of DMATCH arrays (host).
        cross_check: keep a match i -> j only if i is also the nearest query of j (SFMHIP_MATCH_MUTUAL)."""
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n_pairs = pairs.shape[0]
        if n_pairs == 0:
            return []
        mpp = max(1, max(sets[a].rows for a in pairs[:, 0]))
        out = np.empty((n_pairs, mpp), DMATCH)        # (only out[p, :counts[p]] is ever handed out: zero-filling 16 MB cost ~1 ms of a 4 ms chain)
        counts = np.zeros(n_pairs, np.int32)
        arr = (C.c_void_p * len(sets))(*[s.handle for s in sets])
        self._check(self.lib.sfmhip_match_pairs_ex(self.h, arr, len(sets), pairs.ctypes.data, n_pairs, ratio, floor_, mult,
                                                   _lib.MATCH_MUTUAL if cross_check else 0, out.ctypes.data, mpp, counts.ctypes.data))
        # views into the one result buffer (a copy per pair cost 3.8 ms of a 13 ms C4 chain from host rows)
        return [out[p, :c] for p, c in enumerate(counts.tolist())]

    def match_pairs_dev(self, sets, pairs, d_matches, max_per_pair, d_counts, ratio=0.6, floor_=10.0, mult=5.0, cross_check=False):
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        arr = (C.c_void_p * len(sets))(*[s.handle for s in sets])
        self._check(self.lib.sfmhip_match_pairs_ex_dev(self.h, arr, len(sets), pairs.ctypes.data, pairs.shape[0],
                                                       ratio, floor_, mult, _lib.MATCH_MUTUAL if cross_check else 0,
                                                       d_matches.data_ptr(), max_per_pair, d_counts.data_ptr()))

    def l2_distance_matrix_dev(self, qset, tset, dist, force_path=0):
        """dist: torch float32 CUDA tensor (nq, >= nt), row-contiguous; enqueues only."""
        self._check(self.lib.sfmhip_l2_distance_matrix_dev(self.h, qset.handle, tset.handle, dist.data_ptr(),
                                                           dist.stride(0), force_path))

    # ---------------------------------------------------------------- triangulation
    def triangulate2(self, P1, P2, xy1, xy2):
        P1 = np.ascontiguousarray(P1, np.float32).reshape(12); P2 = np.ascontiguousarray(P2, np.float32).reshape(12)
        xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2); xy2 = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
        n = xy1.shape[0]
        xyzw = np.empty((4, n), np.float32); xyz = np.empty((n, 3), np.float64)
        self._check(self.lib.sfmhip_triangulate2_f32(self.h, P1.ctypes.data, P2.ctypes.data, xy1.ctypes.data,
                                                     xy2.ctypes.data, n, xyzw.ctypes.data, xyz.ctypes.data))
        return xyzw, xyz

    def triangulate2_dev(self, P1, P2, xy1, xy2, xyzw, xyz):
        P1 = np.ascontiguousarray(P1, np.float32).reshape(12); P2 = np.ascontiguousarray(P2, np.float32).reshape(12)
        self._check(self.lib.sfmhip_triangulate2_f32_dev(self.h, P1.ctypes.data, P2.ctypes.data, xy1.data_ptr(),
                                                         xy2.data_ptr(), xy1.shape[0], _ptr(xyzw), _ptr(xyz)))

    def triangulate2_matches_dev(self, P1, P2, kp1, kp2, matches, n, xyzw, xyz):
        P1 = np.ascontiguousarray(P1, np.float32).reshape(12); P2 = np.ascontiguousarray(P2, np.float32).reshape(12)
        self._check(self.lib.sfmhip_triangulate2_matches_dev(self.h, P1.ctypes.data, P2.ctypes.data, _ptr(kp1), _ptr(kp2),
                                                             _ptr(matches), n, _ptr(xyzw), _ptr(xyz)))

    # ---------------------------------------------------------------- bundle adjustment
    def triangulate_tracks(self, K4, ext, obs_cam, obs_pt, obs_uv, n_pt):
        """N-view DLT of every track (extension, sfmhip_triangulate_tracks): returns (pts (n_pt,3) float64, n_views int32)."""
        K4 = np.ascontiguousarray(K4, np.float64); ext = np.ascontiguousarray(ext, np.float64)
        oc = np.ascontiguousarray(obs_cam, np.int32); op = np.ascontiguousarray(obs_pt, np.int32); uv = np.ascontiguousarray(obs_uv, np.float64)
        pts = np.empty((n_pt, 3), np.float64); nv = np.empty(n_pt, np.int32)
        self._check(self.lib.sfmhip_triangulate_tracks(self.h, _ptr(K4), _ptr(ext), ext.shape[0], _ptr(oc), _ptr(op), _ptr(uv),
                                                       oc.shape[0], int(n_pt), _ptr(pts), _ptr(nv)))
        return pts, nv

    def reprojection_errors(self, K4, ext, pts, obs_cam, obs_pt, obs_uv):
        """pixel error of every observation (sfmhip_reprojection_errors)"""
        K4 = np.ascontiguousarray(K4, np.float64); ext = np.ascontiguousarray(ext, np.float64); pts = np.ascontiguousarray(pts, np.float64)
        oc = np.ascontiguousarray(obs_cam, np.int32); op = np.ascontiguousarray(obs_pt, np.int32); uv = np.ascontiguousarray(obs_uv, np.float64)
        err = np.empty(oc.shape[0], np.float64)
        self._check(self.lib.sfmhip_reprojection_errors(self.h, _ptr(K4), _ptr(ext), ext.shape[0], _ptr(pts), pts.shape[0],
                                                        _ptr(oc), _ptr(op), _ptr(uv), oc.shape[0], _ptr(err)))
        return err

    def ba_options(self, **kw):
        o = BAOptions()
        self.lib.sfmhip_ba_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def ba_create(self, K4, ext, pts, obs_cam, obs_pt, obs_uv, opts=None, cam_const=None, pt_const=None):
        """cam_const / pt_const: per-camera / per-point flags (bool or uint8), nonzero = constant (sfmhip_ba_create_ex); None: none"""
        return BAProblem(self, K4, ext, pts, obs_cam, obs_pt, obs_uv, opts, cam_const, pt_const)

    def ba_solve(self, K4, ext, pts, obs_cam, obs_pt, obs_uv, opts=None, cam_const=None, pt_const=None):
        """One-shot sfmhip_ba_solve on copies; returns (K4, ext, pts, summary dict).  cam_const / pt_const: as ba_create
        (sfmhip_ba_solve_ex)."""
        K4 = np.array(K4, np.float64).reshape(4).copy(); ext = np.array(ext, np.float64).reshape(-1, 6).copy()
        pts = np.array(pts, np.float64).reshape(-1, 3).copy()
        oc = np.ascontiguousarray(obs_cam, np.int32); op = np.ascontiguousarray(obs_pt, np.int32)
        uv = np.ascontiguousarray(obs_uv, np.float64).reshape(-1, 2)
        o = opts if opts is not None else self.ba_options()
        s = BASummary()
        if cam_const is None and pt_const is None:
            self._check(self.lib.sfmhip_ba_solve(self.h, K4.ctypes.data, ext.ctypes.data, ext.shape[0], pts.ctypes.data,
                                                 pts.shape[0], oc.ctypes.data, op.ctypes.data, uv.ctypes.data, oc.shape[0],
                                                 C.byref(o), C.byref(s)))
        else:
            cm, pm = _const_mask(cam_const, ext.shape[0]), _const_mask(pt_const, pts.shape[0])
            self._check(self.lib.sfmhip_ba_solve_ex(self.h, K4.ctypes.data, ext.ctypes.data, ext.shape[0], pts.ctypes.data,
                                                    pts.shape[0], oc.ctypes.data, op.ctypes.data, uv.ctypes.data, oc.shape[0],
                                                    _mask_ptr(cm), _mask_ptr(pm), C.byref(o), C.byref(s)))
        return K4, ext, pts, s.asdict()

    # ---------------------------------------------------------------- point clouds: neighbours, normals, outlier filter
    @staticmethod
    def _points_method(method):
        """"auto" / "brute" / "grid" or the SFMHIP_POINTS_* number"""
        if isinstance(method, str):
            if method not in _lib.POINTS_METHODS:
                raise ValueError(f"method {method!r}: one of {sorted(_lib.POINTS_METHODS)}")
            return _lib.POINTS_METHODS[method]
        return int(method)

    def knn_points(self, pts, K=10, method="auto"):
        """(idx n x K int32, dist n x K float64): the K nearest OTHER points of every point, ordered by (distance, index);
        -1 / inf where a point has fewer (sfmhip_knn_points).  Exact for every method."""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        n, K = pts.shape[0], int(K)
        idx = np.empty((n, max(K, 0)), np.int32); dist = np.empty((n, max(K, 0)), np.float64)
        self._check(self.lib.sfmhip_knn_points(self.h, pts.ctypes.data, n, K, self._points_method(method), idx.ctypes.data, dist.ctypes.data))
        return idx, dist

    def knn_points_dev(self, d_pts, n, K, d_idx, d_dist, method="auto"):
        """the same on device pointers (integers; 0: not wanted): enqueues on the context's stream, never synchronises"""
        self._check(self.lib.sfmhip_knn_points_dev(self.h, C.c_void_p(int(d_pts)), int(n), int(K), self._points_method(method),
                                                   C.c_void_p(int(d_idx)) if d_idx else None, C.c_void_p(int(d_dist)) if d_dist else None))

    def estimate_normals(self, pts, K=10, method="auto", radius=None):
        """normals from the K nearest neighbours; with a radius, from those of them within it (sfmhip_estimate_normals_hybrid:
        NaN for a point that has none)"""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        out = np.empty_like(pts)
        if radius is None:
            self._check(self.lib.sfmhip_estimate_normals_ex(self.h, pts.ctypes.data, pts.shape[0], int(K), self._points_method(method), out.ctypes.data))
        else:
            self._check(self.lib.sfmhip_estimate_normals_hybrid(self.h, pts.ctypes.data, pts.shape[0], int(K), float(radius),
                                                                self._points_method(method), out.ctypes.data))
        return out

    def statistical_outliers(self, pts, K=10, std_ratio=2.0, method="auto"):
        """(keep bool n, mean_dist float64 n, stats = [mu, sigma, thr]): statistical outlier removal as in PCL / Open3D
        (sfmhip_statistical_outliers); keep == (mean_dist <= thr), thr = mu + std_ratio * sigma over the finite mean distances"""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        n = pts.shape[0]
        keep = np.zeros(n, np.uint8); mean_dist = np.empty(n, np.float64); stats = np.full(3, np.nan)
        self._check(self.lib.sfmhip_statistical_outliers(self.h, pts.ctypes.data, n, int(K), float(std_ratio), self._points_method(method),
                                                         keep.ctypes.data, mean_dist.ctypes.data, stats.ctypes.data))
        return keep.astype(bool), mean_dist, stats

    def radius_count(self, pts, r, method="auto"):
        """count int32 n: the number of OTHER points within distance r (inclusive, on the computed fp64 distance) of every point
        (sfmhip_radius_count); r = 0 counts exact duplicates.  The same counts for every method."""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        count = np.zeros(pts.shape[0], np.int32)
        self._check(self.lib.sfmhip_radius_count(self.h, pts.ctypes.data, pts.shape[0], float(r), self._points_method(method), count.ctypes.data))
        return count

    def radius_count_dev(self, d_pts, n, r, d_count, method="auto"):
        """the same on device pointers (integers): enqueues on the context's stream, never synchronises"""
        self._check(self.lib.sfmhip_radius_count_dev(self.h, C.c_void_p(int(d_pts)), int(n), float(r), self._points_method(method),
                                                     C.c_void_p(int(d_count)) if d_count else None))

    def radius_outliers(self, pts, r, min_neighbors, method="auto"):
        """(keep bool n, count int32 n): radius outlier removal (sfmhip_radius_outliers); keep == (count >= min_neighbors)"""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        n = pts.shape[0]
        keep = np.zeros(n, np.uint8); count = np.zeros(n, np.int32)
        self._check(self.lib.sfmhip_radius_outliers(self.h, pts.ctypes.data, n, float(r), int(min_neighbors), self._points_method(method),
                                                    keep.ctypes.data, count.ctypes.data))
        return keep.astype(bool), count

    def voxel_downsample(self, pts, voxel):
        """(centroids m x 3 float64, counts int32 m, voxel_of int32 n, origin float64 3): one centroid per occupied voxel of edge
        `voxel`, voxels in ascending (c_x, c_y, c_z) (sfmhip_voxel_downsample); voxel_of is -1 for a non-finite point"""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        n = pts.shape[0]
        cen = np.empty((n, 3), np.float64); counts = np.empty(n, np.int32); voxel_of = np.full(n, -1, np.int32)
        origin = np.full(3, np.inf); m = C.c_int(0)
        self._check(self.lib.sfmhip_voxel_downsample(self.h, pts.ctypes.data, n, float(voxel), cen.ctypes.data, counts.ctypes.data,
                                                     voxel_of.ctypes.data, C.byref(m), origin.ctypes.data))
        return cen[:m.value].copy(), counts[:m.value].copy(), voxel_of, origin

    def voxel_downsample_dev(self, d_pts, n, voxel, d_centroids, d_counts, d_voxel_of, d_n_voxels, d_origin=0):
        """the same on device pointers (integers; 0 for d_counts / d_voxel_of / d_origin: not wanted): enqueues on the context's
        stream, never synchronises; the int32 at d_n_voxels becomes -1 where the voxel is too small for the cloud's extent"""
        p = lambda a: C.c_void_p(int(a)) if a else None      # noqa: E731
        self._check(self.lib.sfmhip_voxel_downsample_dev(self.h, p(d_pts), int(n), float(voxel), p(d_centroids), p(d_counts), p(d_voxel_of),
                                                         p(d_n_voxels), p(d_origin)))

    def cluster_dbscan(self, pts, eps, min_points=1, method="auto"):
        """(labels int32 n, sizes int32 C): DBSCAN as in scikit-learn / Open3D's cluster_dbscan (sfmhip_cluster_dbscan): a point with
        at least min_points points within eps of it, itself included, is core; clusters are the connected components of the core
        points, numbered by their smallest core index; a border point takes the smallest number among its core neighbours; noise and
        non-finite points are -1.  min_points = 1: Euclidean cluster extraction.  The same labels for every method."""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        n = pts.shape[0]
        labels = np.full(n, -1, np.int32); sizes = np.zeros(n, np.int32); m = C.c_int(0)
        self._check(self.lib.sfmhip_cluster_dbscan(self.h, pts.ctypes.data, n, float(eps), int(min_points), self._points_method(method),
                                                   labels.ctypes.data, C.byref(m), sizes.ctypes.data, None))
        return labels, sizes[:m.value].copy()

    def cluster_dbscan_dev(self, d_pts, n, eps, min_points, d_labels, d_n_clusters, d_sizes=0, d_count=0, method="auto"):
        """the same on device pointers (integers; 0 for d_sizes / d_count: not wanted): enqueues on the context's stream, never
        synchronises; d_sizes holds n entries, zero from the number of clusters on"""
        p = lambda a: C.c_void_p(int(a)) if a else None      # noqa: E731
        self._check(self.lib.sfmhip_cluster_dbscan_dev(self.h, p(d_pts), int(n), float(eps), int(min_points), self._points_method(method),
                                                       p(d_labels), p(d_n_clusters), p(d_sizes), p(d_count)))

    def largest_cluster(self, pts, eps, min_points=1, method="auto"):
        """(keep bool n, labels int32 n, sizes int32 C): keep marks the cluster with the most points, the smallest number among equals
        (sfmhip_largest_cluster); all False where there is no cluster"""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        n = pts.shape[0]
        keep = np.zeros(n, np.uint8); labels = np.full(n, -1, np.int32); m = C.c_int(0); big = C.c_int(0)
        self._check(self.lib.sfmhip_largest_cluster(self.h, pts.ctypes.data, n, float(eps), int(min_points), self._points_method(method),
                                                    keep.ctypes.data, labels.ctypes.data, C.byref(m), C.byref(big)))
        sizes = np.bincount(labels[labels >= 0], minlength=m.value).astype(np.int32)
        return keep.astype(bool), labels, sizes

    def segment_planes(self, pts, threshold, max_planes=1, hypotheses=1024, seed=0, min_inliers=3):
        """(labels int32 n, planes P x 4, counts int32 P, winner int32 P, refined P x 4): RANSAC plane segmentation as in Open3D's
        segment_plane / PCL's SACSegmentation, up to max_planes planes peeled off one after another (sfmhip_segment_planes, where the
        definition is).  labels: the plane number or -1; planes: (a, b, c, d) of the winning hypothesis, d >= 0; refined: the
        least-squares plane of each plane's inliers.  P is the number of planes found.  Every integer output depends on the input alone."""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        n, mp = pts.shape[0], int(max_planes)
        cap = max(mp, 0)
        labels = np.full(n, -1, np.int32); planes = np.full((cap, 4), np.nan); refined = np.full((cap, 4), np.nan)
        counts = np.zeros(cap, np.int32); winner = np.full(cap, -1, np.int32); m = C.c_int(0)
        self._check(self.lib.sfmhip_segment_planes(self.h, pts.ctypes.data, n, float(threshold), int(hypotheses), int(seed) & (2 ** 64 - 1),
                                                   int(min_inliers), mp, labels.ctypes.data, C.byref(m), planes.ctypes.data, refined.ctypes.data,
                                                   counts.ctypes.data, winner.ctypes.data))
        P = m.value
        return labels, planes[:P].copy(), counts[:P].copy(), winner[:P].copy(), refined[:P].copy()

    def segment_planes_dev(self, d_pts, n, threshold, max_planes, d_labels, d_n_planes, d_planes, d_refined=0, d_counts=0, d_winner=0,
                           hypotheses=1024, seed=0, min_inliers=3):
        """the same on device pointers (integers; 0 for d_refined / d_counts / d_winner: not wanted): enqueues on the context's stream,
        never synchronises; the per-plane arrays hold max_planes rows, NaN / 0 / -1 from the number of planes on"""
        p = lambda a: C.c_void_p(int(a)) if a else None      # noqa: E731
        self._check(self.lib.sfmhip_segment_planes_dev(self.h, p(d_pts), int(n), float(threshold), int(hypotheses), int(seed) & (2 ** 64 - 1),
                                                       int(min_inliers), int(max_planes), p(d_labels), p(d_n_planes), p(d_planes), p(d_refined),
                                                       p(d_counts), p(d_winner)))

    def segment_plane(self, pts, threshold, hypotheses=1024, seed=0, min_inliers=3):
        """(plane float64 4, keep bool n, refined float64 4): the dominant plane as a filter (sfmhip_segment_plane); no plane found:
        NaN planes and keep all False"""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        n = pts.shape[0]
        plane = np.full(4, np.nan); refined = np.full(4, np.nan); keep = np.zeros(n, np.uint8); cnt = C.c_int(0)
        self._check(self.lib.sfmhip_segment_plane(self.h, pts.ctypes.data, n, float(threshold), int(hypotheses), int(seed) & (2 ** 64 - 1),
                                                  int(min_inliers), plane.ctypes.data, keep.ctypes.data, C.byref(cnt), refined.ctypes.data))
        return plane, keep.astype(bool), refined

    # ---------------------------------------------------------------- two-view geometric verification
    def verify_pairs(self, corr_blocks, t, hypotheses=1024, rounds=3, seed=0, min_inliers=8):
        """(masks, counts int32 n, F n x 3 x 3, winner int32 n): the epipolar RANSAC of sfmhip_verify_pairs (where the definition is) on
        every block of corr_blocks, a sequence of (m_q, 4) arrays of rows (x1, y1, x2, y2), all pairs in one call.  masks[q]: bool m_q,
        the rows the pair's model accepts; counts[q] = masks[q].sum(), 0 (with NaN F and winner -1) where no model reaches min_inliers.
        Every output depends on the pair's own rows alone."""
        blocks = [np.ascontiguousarray(b, np.float64).reshape(-1, 4) for b in corr_blocks]
        n = len(blocks)
        counts = np.array([len(b) for b in blocks], np.int32)
        stride = int(counts.max()) if n else 0
        corr = np.zeros((n, stride, 4))
        for q, b in enumerate(blocks):
            corr[q, :len(b)] = b
        mask = np.zeros((n, stride), np.uint8); cnt = np.zeros(n, np.int32); F = np.full((n, 9), np.nan); win = np.full(n, -1, np.int32)
        self._check(self.lib.sfmhip_verify_pairs(self.h, corr.ctypes.data, stride, counts.ctypes.data, n, float(t), int(hypotheses), int(rounds),
                                                 int(seed) & (2 ** 64 - 1), int(min_inliers), mask.ctypes.data, cnt.ctypes.data, F.ctypes.data,
                                                 win.ctypes.data))
        return [mask[q, :c].astype(bool) for q, c in enumerate(counts.tolist())], cnt, F.reshape(n, 3, 3), win

    def verify_pairs_dev(self, d_corr, stride, d_counts, n_pairs, t, d_mask, d_count_out, d_F=0, d_winner=0, hypotheses=1024, rounds=3, seed=0,
                         min_inliers=8):
        """the same on device arrays (torch tensors or integer addresses; 0 for d_F / d_winner: not wanted): d_corr n_pairs x stride x 4
        float64, d_counts int32, d_mask n_pairs x stride uint8, d_count_out int32; enqueues on the context's stream, never synchronises"""
        self._check(self.lib.sfmhip_verify_pairs_dev(self.h, _dptr(d_corr), int(stride), _dptr(d_counts), int(n_pairs), float(t), int(hypotheses),
                                                     int(rounds), int(seed) & (2 ** 64 - 1), int(min_inliers), _dptr(d_mask), _dptr(d_count_out),
                                                     _dptr(d_F), _dptr(d_winner)))

    def verify_matches_dev(self, d_kp, pairs, K4, d_matches, max_per_pair, d_counts, t, d_matches_out, d_counts_out, d_F=0, d_winner=0,
                           hypotheses=1024, rounds=3, seed=0, min_inliers=8):
        """the match lists of match_pairs_dev verified on the device (sfmhip_verify_matches_dev): d_kp: one device KEYPOINT array per image
        (torch tensors or addresses); pairs (n_pairs, 2); K4 = (fx, fy, cx, cy), (1, 1, 0, 0) for pixel coordinates; d_matches_out /
        d_counts_out: the surviving elements in the layout of the input, for triangulate2_matches_dev.  Enqueues only."""
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        K4 = np.ascontiguousarray(K4, np.float64).reshape(4)
        arr = (C.c_void_p * len(d_kp))(*[_dptr(k) for k in d_kp])
        self._check(self.lib.sfmhip_verify_matches_dev(self.h, arr, len(d_kp), pairs.ctypes.data, pairs.shape[0], K4.ctypes.data, _dptr(d_matches),
                                                       int(max_per_pair), _dptr(d_counts), float(t), int(hypotheses), int(rounds),
                                                       int(seed) & (2 ** 64 - 1), int(min_inliers), _dptr(d_matches_out), _dptr(d_counts_out),
                                                       _dptr(d_F), _dptr(d_winner)))

    # ---------------------------------------------------------------- homography RANSAC and F/H model selection
    @staticmethod
    def _corr_blocks(corr_blocks):
        """(corr n x stride x 4, counts int32 n, n, stride) of a sequence of (m_q, 4) arrays"""
        blocks = [np.ascontiguousarray(b, np.float64).reshape(-1, 4) for b in corr_blocks]
        n = len(blocks)
        counts = np.array([len(b) for b in blocks], np.int32)
        stride = int(counts.max()) if n else 0
        corr = np.zeros((n, stride, 4))
        for q, b in enumerate(blocks):
            corr[q, :len(b)] = b
        return corr, counts, n, stride

    def verify_pairs_h(self, corr_blocks, t, hypotheses=1024, rounds=3, seed=0, min_inliers=4):
        """(masks, counts int32 n, Hm n x 3 x 3, winner int32 n): the four-point homography RANSAC of sfmhip_verify_pairs_h on every block
        of corr_blocks, in the form of verify_pairs; Hm maps image 1 to image 2."""
        corr, counts, n, stride = self._corr_blocks(corr_blocks)
        mask = np.zeros((n, stride), np.uint8); cnt = np.zeros(n, np.int32); Hm = np.full((n, 9), np.nan); win = np.full(n, -1, np.int32)
        self._check(self.lib.sfmhip_verify_pairs_h(self.h, corr.ctypes.data, stride, counts.ctypes.data, n, float(t), int(hypotheses), int(rounds),
                                                   int(seed) & (2 ** 64 - 1), int(min_inliers), mask.ctypes.data, cnt.ctypes.data, Hm.ctypes.data,
                                                   win.ctypes.data))
        return [mask[q, :c].astype(bool) for q, c in enumerate(counts.tolist())], cnt, Hm.reshape(n, 3, 3), win

    def verify_pairs_h_dev(self, d_corr, stride, d_counts, n_pairs, t, d_mask, d_count_out, d_Hm=0, d_winner=0, hypotheses=1024, rounds=3, seed=0,
                           min_inliers=4):
        """the same on device arrays, in the form of verify_pairs_dev; enqueues only"""
        self._check(self.lib.sfmhip_verify_pairs_h_dev(self.h, _dptr(d_corr), int(stride), _dptr(d_counts), int(n_pairs), float(t), int(hypotheses),
                                                       int(rounds), int(seed) & (2 ** 64 - 1), int(min_inliers), _dptr(d_mask), _dptr(d_count_out),
                                                       _dptr(d_Hm), _dptr(d_winner)))

    # ---------------------------------------------------------------- two-view relative pose
    def relative_pose(self, blocks, masks, F, t, rounds=3, iters=10, max_depth=50.0, min_angle_deg=2.0):
        """(pose n x 12, info int32 n x 10, quality n x 5, masks_out): the relative pose of sfmhip_relative_pose (where the definition
        is) for every block of blocks, a sequence of (m_q, 4) arrays of rows (x1, y1, x2, y2) NORMALISED by K, all pairs in one call.
        masks: per pair the bool / uint8 inlier mask of verify_pairs or two_view_geometry, or None for every row; F: n x 3 x 3, the
        epipolar model on those rows; t: the Sampson threshold.  pose[q] = R row-major then the unit t (NaN without a pose);
        info[q] = status, cand, n4[0..3], n_used, n_inl, n_front, n_angle; quality[q] = s0, s1, s2, cost before and after the last
        round; masks_out[q]: uint8 m_q, bit 0 the final Sampson inlier, bit 1 in front of both cameras, bit 2 the parallax."""
        corr, counts, n, stride = self._corr_blocks(blocks)
        F = np.ascontiguousarray(F, np.float64).reshape(n, 9)
        mask_in = None
        if masks is not None:
            mask_in = np.zeros((n, stride), np.uint8)
            for q, m in enumerate(masks):
                m = np.asarray(m).reshape(-1)
                if len(m) != counts[q]:
                    raise ValueError(f"mask {q} has {len(m)} entries for {counts[q]} rows")
                mask_in[q, :len(m)] = m != 0
        pose = np.full((n, 12), np.nan); info = np.zeros((n, 10), np.int32); quality = np.full((n, 5), np.nan); mask = np.zeros((n, stride), np.uint8)
        self._check(self.lib.sfmhip_relative_pose(self.h, corr.ctypes.data, stride, counts.ctypes.data, n, mask_in.ctypes.data if mask_in is not None else None,
                                                  F.ctypes.data, float(t), int(rounds), int(iters), float(max_depth), float(np.radians(min_angle_deg)),
                                                  pose.ctypes.data, info.ctypes.data, quality.ctypes.data, mask.ctypes.data))
        return pose, info, quality, [mask[q, :c].copy() for q, c in enumerate(counts.tolist())]

    def relative_pose_dev(self, d_corr, stride, d_counts, n_pairs, d_mask_in, d_F, t, d_pose, d_info, d_quality=0, d_mask_out=0, rounds=3, iters=10,
                          max_depth=50.0, min_angle_deg=2.0):
        """the same on device arrays (torch tensors or integer addresses; 0 for d_mask_in: every row, for d_quality / d_mask_out: not
        wanted): d_corr n_pairs x stride x 4 float64, d_mask_in / d_mask_out n_pairs x stride uint8, d_F n_pairs x 9, d_pose n_pairs x 12,
        d_info int32 n_pairs x 10, d_quality n_pairs x 5; one kernel launch on the context's stream, never synchronises"""
        self._check(self.lib.sfmhip_relative_pose_dev(self.h, _dptr(d_corr), int(stride), _dptr(d_counts), int(n_pairs), _dptr(d_mask_in), _dptr(d_F),
                                                      float(t), int(rounds), int(iters), float(max_depth), float(np.radians(min_angle_deg)),
                                                      _dptr(d_pose), _dptr(d_info), _dptr(d_quality), _dptr(d_mask_out)))

    # ---------------------------------------------------------------- image registration (absolute pose)
    def register_views(self, blocks, t, hypotheses=1024, rounds=3, seed=0, min_inliers=6):
        """(masks, counts int32 n, P n x 3 x 4, winner int32 n): the six-point DLT RANSAC of sfmhip_register_views (where the definition
        is) on every block of blocks, a sequence of (m_q, 5) arrays of rows (X, Y, Z, x, y), all views in one call.  masks[q]: bool m_q,
        the rows the view's model accepts; counts[q] = masks[q].sum(), 0 (with NaN P and winner -1) where no model reaches min_inliers.
        pose_from_projection turns a P on normalised observations into a pose."""
        rows = [np.ascontiguousarray(b, np.float64).reshape(-1, 5) for b in blocks]
        n = len(rows)
        counts = np.array([len(b) for b in rows], np.int32)
        stride = int(counts.max()) if n else 0
        corr = np.zeros((n, stride, 5))
        for q, b in enumerate(rows):
            corr[q, :len(b)] = b
        mask = np.zeros((n, stride), np.uint8); cnt = np.zeros(n, np.int32); P = np.full((n, 12), np.nan); win = np.full(n, -1, np.int32)
        self._check(self.lib.sfmhip_register_views(self.h, corr.ctypes.data, stride, counts.ctypes.data, n, float(t), int(hypotheses), int(rounds),
                                                   int(seed) & (2 ** 64 - 1), int(min_inliers), mask.ctypes.data, cnt.ctypes.data, P.ctypes.data,
                                                   win.ctypes.data))
        return [mask[q, :c].astype(bool) for q, c in enumerate(counts.tolist())], cnt, P.reshape(n, 3, 4), win

    def register_views_dev(self, d_corr, stride, d_counts, n_views, t, d_mask, d_count_out, d_P=0, d_winner=0, hypotheses=1024, rounds=3, seed=0,
                           min_inliers=6):
        """the same on device arrays, in the form of verify_pairs_dev (d_corr n_views x stride x 5 float64, d_P n_views x 12); enqueues only"""
        self._check(self.lib.sfmhip_register_views_dev(self.h, _dptr(d_corr), int(stride), _dptr(d_counts), int(n_views), float(t), int(hypotheses),
                                                       int(rounds), int(seed) & (2 ** 64 - 1), int(min_inliers), _dptr(d_mask), _dptr(d_count_out),
                                                       _dptr(d_P), _dptr(d_winner)))

    def two_view_geometry(self, corr_blocks, t_f, t_h, hypotheses=1024, rounds=3, seed=0, min_inliers=8, hf_ratio=0.8):
        """(kind int32 n, masks, counts int32 n, counts2 int32 n x 2, F n x 3 x 3, Hm n x 3 x 3, winners int32 n x 2): both RANSACs and
        the selection of sfmhip_two_view_geometry.  kind 0: no model, 1: general (masks[q], counts[q] are F's), 2: planar or panoramic
        (they are the homography's); counts2, F, Hm and winners report both models whatever the kind."""
        corr, counts, n, stride = self._corr_blocks(corr_blocks)
        kind = np.zeros(n, np.int32); mask = np.zeros((n, stride), np.uint8); cnt = np.zeros(n, np.int32); c2 = np.zeros((n, 2), np.int32)
        F = np.full((n, 9), np.nan); Hm = np.full((n, 9), np.nan); win = np.full((n, 2), -1, np.int32)
        self._check(self.lib.sfmhip_two_view_geometry(self.h, corr.ctypes.data, stride, counts.ctypes.data, n, float(t_f), float(t_h), int(hypotheses),
                                                      int(rounds), int(seed) & (2 ** 64 - 1), int(min_inliers), float(hf_ratio), kind.ctypes.data,
                                                      mask.ctypes.data, cnt.ctypes.data, c2.ctypes.data, F.ctypes.data, Hm.ctypes.data, win.ctypes.data))
        return kind, [mask[q, :c].astype(bool) for q, c in enumerate(counts.tolist())], cnt, c2, F.reshape(n, 3, 3), Hm.reshape(n, 3, 3), win

    def two_view_geometry_dev(self, d_corr, stride, d_counts, n_pairs, t_f, t_h, d_kind, d_mask, d_count_out, d_counts2=0, d_F=0, d_Hm=0, d_winners=0,
                              hypotheses=1024, rounds=3, seed=0, min_inliers=8, hf_ratio=0.8):
        """the same on device arrays (0: not wanted): d_kind int32 n_pairs, d_counts2 / d_winners int32 n_pairs x 2; enqueues only, no
        round and no selection waits on the host"""
        self._check(self.lib.sfmhip_two_view_geometry_dev(self.h, _dptr(d_corr), int(stride), _dptr(d_counts), int(n_pairs), float(t_f), float(t_h),
                                                          int(hypotheses), int(rounds), int(seed) & (2 ** 64 - 1), int(min_inliers), float(hf_ratio),
                                                          _dptr(d_kind), _dptr(d_mask), _dptr(d_count_out), _dptr(d_counts2), _dptr(d_F), _dptr(d_Hm),
                                                          _dptr(d_winners)))

    def two_view_geometry_matches_dev(self, d_kp, pairs, K4, d_matches, max_per_pair, d_counts, t_f, t_h, d_kind, d_matches_out, d_counts_out,
                                      d_counts2=0, d_F=0, d_Hm=0, d_winners=0, hypotheses=1024, rounds=3, seed=0, min_inliers=8, hf_ratio=0.8):
        """verify_matches_dev with the selection (sfmhip_two_view_geometry_matches_dev): d_matches_out / d_counts_out receive the elements
        the selected model of every pair keeps, for triangulate2_matches_dev; d_kind says which model that was.  Enqueues only."""
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        K4 = np.ascontiguousarray(K4, np.float64).reshape(4)
        arr = (C.c_void_p * len(d_kp))(*[_dptr(k) for k in d_kp])
        self._check(self.lib.sfmhip_two_view_geometry_matches_dev(self.h, arr, len(d_kp), pairs.ctypes.data, pairs.shape[0], K4.ctypes.data,
                                                                  _dptr(d_matches), int(max_per_pair), _dptr(d_counts), float(t_f), float(t_h),
                                                                  int(hypotheses), int(rounds), int(seed) & (2 ** 64 - 1), int(min_inliers),
                                                                  float(hf_ratio), _dptr(d_kind), _dptr(d_matches_out), _dptr(d_counts_out),
                                                                  _dptr(d_counts2), _dptr(d_F), _dptr(d_Hm), _dptr(d_winners)))

    # ---------------------------------------------------------------- SIFT on the device
    @staticmethod
    def _image(img):
        """(array, rows, cols, channels, ld bytes) of a uint8 image rows x cols (gray) or rows x cols x 3 (BGR); a padded row stride is
        kept (the columns must be dense)"""
        a = np.asarray(img)
        if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)):
            raise ValueError("an image is a uint8 array rows x cols or rows x cols x 3")
        ch = 1 if a.ndim == 2 else a.shape[2]
        dense = a.strides[1] == ch and (a.ndim == 2 or a.strides[2] == 1) and a.strides[0] >= a.shape[1] * ch
        if not dense or a.shape[0] == 0 or a.shape[1] == 0:
            a = np.ascontiguousarray(a)
        return a, a.shape[0], a.shape[1], ch, (a.strides[0] if a.shape[0] and a.shape[1] else a.shape[1] * ch)

    def sift_extract(self, img, max_features=0, cap=None):
        """(keypoints[KEYPOINT], descriptors float32 n x 128) of a uint8 image, gray or BGR (sfmhip_sift_extract: the host extractor's
        SIFT, cv::SIFT::create(max_features, 3, 0.04, 10), on the device).  cap: rows the call may write (default: enough; a smaller
        one returns the first cap rows)."""
        a, rows, cols, ch, ld = self._image(img)
        want = int(cap) if cap is not None else (int(max_features) if max_features > 0 else 8192)
        while True:
            kp = np.zeros(max(want, 0), KEYPOINT); desc = np.zeros((max(want, 0), 128), np.float32); n = C.c_int32(0)
            self._check(self.lib.sfmhip_sift_extract(self.h, a.ctypes.data, rows, cols, ch, ld, int(max_features), kp.ctypes.data, desc.ctypes.data,
                                                     want, C.byref(n)))
            if cap is not None or n.value <= want:
                m = min(n.value, max(want, 0))
                return kp[:m].copy(), desc[:m].copy()
            want = n.value

    def sift_extract_dev(self, d_img, d_kp, d_desc, d_n_found, max_features=0, cap=None):
        """the same on torch CUDA tensors: d_img uint8 rows x cols (x 3), d_kp a uint8 tensor of cap x 28 bytes (KEYPOINT rows), d_desc
        float32 cap x 128, d_n_found one int32 (-1: an internal list overflowed).  Enqueues on the context's stream, never synchronises."""
        assert d_img.is_cuda and d_img.dim() in (2, 3) and d_img.stride(-1) == 1
        rows, cols = d_img.shape[0], d_img.shape[1]
        ch = 1 if d_img.dim() == 2 else d_img.shape[2]
        assert d_img.stride(1) == ch
        cap = d_desc.shape[0] if cap is None else int(cap)
        self._check(self.lib.sfmhip_sift_extract_dev(self.h, _dptr(d_img), rows, cols, ch, d_img.stride(0), int(max_features), _dptr(d_kp), _dptr(d_desc),
                                                     cap, _dptr(d_n_found)))

    def sift_scale_space(self, img, octave, index, kind=0):
        """(level float32 rows x cols, n_oct): Gaussian (kind 0, index 0..5) or DoG (kind 1, index 0..4) level of an octave (test helper)"""
        a, rows, cols, ch, ld = self._image(img)
        r, c, no = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self.lib.sfmhip_sift_scale_space(self.h, a.ctypes.data, rows, cols, ch, ld, int(octave), int(index), int(kind), None, r, c, no))
        out = np.empty((r.value, c.value), np.float32)
        self._check(self.lib.sfmhip_sift_scale_space(self.h, a.ctypes.data, rows, cols, ch, ld, int(octave), int(index), int(kind), out.ctypes.data, r, c, no))
        return out, no.value

    def sift_octaves(self, img):
        """number of octaves the scale space of this image has"""
        a, rows, cols, ch, ld = self._image(img)
        no = C.c_int(0)
        self._check(self.lib.sfmhip_sift_scale_space(self.h, a.ctypes.data, rows, cols, ch, ld, 0, 0, 0, None, None, None, no))
        return no.value

    def sift_extrema(self, img, cap=1 << 16):
        """(xysr float32 n x 4, olrc int32 n x 4): the refined DoG extrema before orientation assignment, in (octave, layer, r, c) order
        (test helper)"""
        a, rows, cols, ch, ld = self._image(img)
        xysr = np.zeros((cap, 4), np.float32); olrc = np.zeros((cap, 4), np.int32); n = C.c_int32(0)
        self._check(self.lib.sfmhip_sift_extrema(self.h, a.ctypes.data, rows, cols, ch, ld, xysr.ctypes.data, olrc.ctypes.data, int(cap), C.byref(n)))
        m = min(n.value, cap)
        return xysr[:m].copy(), olrc[:m].copy()

    def sift_extract_for_all(self, images, max_features=0):
        """extract_features' loop (NViewReconstuct.cpp:785-848) on this context: [(keypoints, descriptors)] image by image"""
        return [self.sift_extract(img, max_features) for img in images]

    # ---------------------------------------------------------------- AKAZE on the device
    def akaze_extract(self, img, max_features=0, cap=None):
        """(keypoints[KEYPOINT], descriptors uint8 n x 61) of a uint8 image, gray or BGR (sfmhip_akaze_extract: the host extractor's
        AKAZE, cv::AKAZE::create(), on the device).  cap: rows the call may write (default: enough; a smaller one returns the first
        cap rows)."""
        a, rows, cols, ch, ld = self._image(img)
        want = int(cap) if cap is not None else (int(max_features) if max_features > 0 else 8192)
        while True:
            kp = np.zeros(max(want, 0), KEYPOINT); desc = np.zeros((max(want, 0), 61), np.uint8); n = C.c_int32(0)
            self._check(self.lib.sfmhip_akaze_extract(self.h, a.ctypes.data, rows, cols, ch, ld, int(max_features), kp.ctypes.data, desc.ctypes.data,
                                                      want, C.byref(n)))
            if cap is not None or n.value <= want:
                m = min(n.value, max(want, 0))
                return kp[:m].copy(), desc[:m].copy()
            want = n.value

    def akaze_extract_dev(self, d_img, d_kp, d_desc, d_n_found, max_features=0, cap=None):
        """the same on torch CUDA tensors: d_img uint8 rows x cols (x 3), d_kp a uint8 tensor of cap x 28 bytes (KEYPOINT rows), d_desc
        uint8 cap x 61 (dense), d_n_found one int32 (-1: the list of raw maxima overflowed).  Enqueues on the context's stream, never
        synchronises."""
        assert d_img.is_cuda and d_img.dim() in (2, 3) and d_img.stride(-1) == 1
        rows, cols = d_img.shape[0], d_img.shape[1]
        ch = 1 if d_img.dim() == 2 else d_img.shape[2]
        assert d_img.stride(1) == ch and d_desc.is_contiguous() and d_desc.shape[1] == 61
        cap = d_desc.shape[0] if cap is None else int(cap)
        self._check(self.lib.sfmhip_akaze_extract_dev(self.h, _dptr(d_img), rows, cols, ch, d_img.stride(0), int(max_features), _dptr(d_kp), _dptr(d_desc),
                                                      cap, _dptr(d_n_found)))

    def akaze_levels(self, img):
        """number of levels the scale space of this image has (0: an octave needs 80 rows and 80 columns)"""
        a, rows, cols, ch, ld = self._image(img)
        nl = C.c_int(0)
        self._check(self.lib.sfmhip_akaze_scale_space(self.h, a.ctypes.data, rows, cols, ch, ld, 0, 0, None, None, None, nl, None))
        return nl.value

    def akaze_scale_space(self, img, level, kind=0):
        """(array float32 rows x cols, n_levels, kcontrast): Lt, Lsmooth, Lx, Ly or Ldet (kind 0 .. 4) of a level (test helper)"""
        a, rows, cols, ch, ld = self._image(img)
        r, c, nl, kc = C.c_int(0), C.c_int(0), C.c_int(0), C.c_float(0)
        self._check(self.lib.sfmhip_akaze_scale_space(self.h, a.ctypes.data, rows, cols, ch, ld, int(level), int(kind), None, r, c, nl, None))
        out = np.empty((r.value, c.value), np.float32)
        self._check(self.lib.sfmhip_akaze_scale_space(self.h, a.ctypes.data, rows, cols, ch, ld, int(level), int(kind), out.ctypes.data, r, c, nl, kc))
        return out, nl.value, np.float32(kc.value)

    def akaze_extrema(self, img, stage=2, cap=1 << 16):
        """(xysr float32 n x 4, ol int32 n x 2 = octave, level): the raw maxima in scan order (stage 0), the survivors of the suppression
        (1) or of the sub-pixel fit (2), in the host's order (test helper)"""
        a, rows, cols, ch, ld = self._image(img)
        xysr = np.zeros((cap, 4), np.float32); ol = np.zeros((cap, 2), np.int32); n = C.c_int32(0)
        self._check(self.lib.sfmhip_akaze_extrema(self.h, a.ctypes.data, rows, cols, ch, ld, int(stage), xysr.ctypes.data, ol.ctypes.data, int(cap), C.byref(n)))
        m = min(n.value, cap)
        return xysr[:m].copy(), ol[:m].copy()

    def akaze_suppress(self, xyr, level):
        """indices (int32) of the candidates {x, y, response} (n x 3) with levels `level` (0 .. 15, not decreasing) that both passes of the
        host's find_extrema keep, in its order (test helper)"""
        xyr = np.ascontiguousarray(xyr, np.float32).reshape(-1, 3)
        level = np.ascontiguousarray(level, np.int32).reshape(-1)
        if len(level) != len(xyr):
            raise ValueError("one level per candidate")
        kept = np.zeros(max(len(xyr), 1), np.int32); n = C.c_int32(0)
        self._check(self.lib.sfmhip_akaze_suppress(self.h, xyr.ctypes.data, level.ctypes.data, len(xyr), kept.ctypes.data, C.byref(n)))
        return kept[:n.value].copy()

    def akaze_extract_for_all(self, images, max_features=0):
        """extract_features' loop (NViewReconstuct.cpp:785-848) with its live extractor on this context: [(keypoints, descriptors)]"""
        return [self.akaze_extract(img, max_features) for img in images]

    # ---------------------------------------------------------------- baseline JPEG on the device
    def jpeg_decode(self, data, entropy=0):
        """uint8 rows x cols (gray) or rows x cols x 3 (BGR, as cv::imread returns it) of a baseline JPEG file's bytes (bytes or a uint8
        array): sfmhip_jpeg_decode, the host decoder's pixels byte for byte.  entropy: 0 automatic, 1 Huffman stage on the host, 2 on
        the device.  SfmHipError for a file the decoder refuses."""
        buf = _jpeg_bytes(data)
        rows, cols, ch, _, _ = jpeg_info(buf)
        out = np.empty((rows, cols) if ch == 1 else (rows, cols, 3), np.uint8)
        self._check(self.lib.sfmhip_jpeg_decode(self.h, buf.ctypes.data, buf.size, int(entropy), out.ctypes.data, cols * ch))
        return out

    def jpeg_decode_dev(self, data, entropy=0):
        """(image, status): the same into a new torch uint8 CUDA tensor, and one int32 that is non-zero when the device entropy stage met
        a corrupt stream (the image is then unspecified).  Enqueues on the context's stream, never synchronises: this is the image
        sift_extract_dev / akaze_extract_dev take."""
        import torch
        buf = _jpeg_bytes(data)
        rows, cols, ch, _, _ = jpeg_info(buf)
        dev = torch.device("cuda", self.device)
        img = torch.empty((rows, cols) if ch == 1 else (rows, cols, 3), dtype=torch.uint8, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        self._check(self.lib.sfmhip_jpeg_decode_dev(self.h, buf.ctypes.data, buf.size, int(entropy), _dptr(img), cols * ch, _dptr(status)))
        return img, status

    # ---------------------------------------------------------------- dense depth (sfmhip_plane_sweep and what follows it)
    def sweep_geometry(self, K4, ext_ref, ext_src):
        """(A float32 n x 9, b float32 n x 3, Rrel n x 9, trel n x 3, Rinv 9, c 3) of sfmhip_sweep_geometry: what the three dense stages
        take instead of poses.  ext: the bundle adjustment's (angle-axis, t) rows; host only"""
        return sweep_geometry(K4, ext_ref, ext_src)

    def plane_sweep(self, ref, srcs, A, b, planes, wmin, wmax, radius=2, min_sources=1, min_score=0.0):
        """(plane int32, score float32, depth float32), each rows x cols: sfmhip_plane_sweep (where the definition is) of the reference
        image against the source images (uint8 rows x cols or rows x cols x 3 BGR; rows of a padded buffer may be passed as a view)"""
        imgs, ptrs, rows, cols, ch, ld = _dense_images([ref] + list(srcs))
        n = len(imgs) - 1
        A = np.ascontiguousarray(A, np.float32).reshape(n, 9); b = np.ascontiguousarray(b, np.float32).reshape(n, 3)
        plane = np.empty((rows, cols), np.int32); score = np.empty((rows, cols), np.float32); depth = np.empty((rows, cols), np.float32)
        src = (C.c_void_p * max(n, 1))(*ptrs[1:])
        self._check(self.lib.sfmhip_plane_sweep(self.h, ptrs[0], src, n, rows, cols, ch, ld, A.ctypes.data, b.ctypes.data, int(planes), float(wmin), float(wmax),
                                                int(radius), int(min_sources), float(min_score), plane.ctypes.data, score.ctypes.data, depth.ctypes.data))
        return plane, score, depth

    def plane_sweep_dev(self, d_ref, d_srcs, rows, cols, channels, ld, A, b, planes, wmin, wmax, radius, min_sources, min_score, d_plane, d_score, d_depth):
        """the same on resident images (torch CUDA tensors or device addresses; A and b stay host arrays): enqueues on the context's
        stream, never synchronises"""
        n = len(d_srcs)
        A = np.ascontiguousarray(A, np.float32).reshape(n, 9); b = np.ascontiguousarray(b, np.float32).reshape(n, 3)
        src = (C.c_void_p * max(n, 1))(*[_dptr(x) for x in d_srcs])
        self._check(self.lib.sfmhip_plane_sweep_dev(self.h, _dptr(d_ref), src, n, int(rows), int(cols), int(channels), int(ld), A.ctypes.data, b.ctypes.data,
                                                    int(planes), float(wmin), float(wmax), int(radius), int(min_sources), float(min_score), _dptr(d_plane),
                                                    _dptr(d_score), _dptr(d_depth)))

    def depth_consistency(self, depth, depth_srcs, K4, Rrel, trel, rel_tol=0.01, min_consistent=1):
        """(count uint8, keep uint8), each rows x cols: sfmhip_depth_consistency of a view's depth map against those of its sources"""
        maps = [np.ascontiguousarray(d, np.float32) for d in [depth] + list(depth_srcs)]
        rows, cols = maps[0].shape
        if any(m.shape != (rows, cols) for m in maps):
            raise ValueError("the depth maps differ in size")
        n = len(maps) - 1
        K4 = np.ascontiguousarray(K4, np.float64).reshape(4); Rrel = np.ascontiguousarray(Rrel, np.float64).reshape(n, 9)
        trel = np.ascontiguousarray(trel, np.float64).reshape(n, 3)
        count = np.empty((rows, cols), np.uint8); keep = np.empty((rows, cols), np.uint8)
        src = (C.c_void_p * max(n, 1))(*[m.ctypes.data for m in maps[1:]])
        self._check(self.lib.sfmhip_depth_consistency(self.h, maps[0].ctypes.data, src, n, rows, cols, K4.ctypes.data, Rrel.ctypes.data, trel.ctypes.data,
                                                      float(rel_tol), int(min_consistent), count.ctypes.data, keep.ctypes.data))
        return count, keep

    def depth_consistency_dev(self, d_depth, d_depth_srcs, rows, cols, K4, Rrel, trel, rel_tol, min_consistent, d_count, d_keep):
        """the same on resident depth maps (K4, Rrel, trel stay host arrays): enqueues only"""
        n = len(d_depth_srcs)
        K4 = np.ascontiguousarray(K4, np.float64).reshape(4); Rrel = np.ascontiguousarray(Rrel, np.float64).reshape(n, 9)
        trel = np.ascontiguousarray(trel, np.float64).reshape(n, 3)
        src = (C.c_void_p * max(n, 1))(*[_dptr(x) for x in d_depth_srcs])
        self._check(self.lib.sfmhip_depth_consistency_dev(self.h, _dptr(d_depth), src, n, int(rows), int(cols), K4.ctypes.data, Rrel.ctypes.data, trel.ctypes.data,
                                                          float(rel_tol), int(min_consistent), _dptr(d_count), _dptr(d_keep)))

    def depth_to_points(self, depth, keep, img, K4, Rinv, c, cap=None):
        """(xyz m x 3 float64, bgr m x 3 uint8, n_found): the kept pixels as world points with their colours, in row-major order
        (sfmhip_depth_to_points); m = min(n_found, cap), cap = every pixel unless given"""
        depth = np.ascontiguousarray(depth, np.float32); keep = np.ascontiguousarray(keep, np.uint8)
        (im,), (ptr,), rows, cols, ch, ld = _dense_images([img])
        if depth.shape != (rows, cols) or keep.shape != (rows, cols):
            raise ValueError("depth, keep and the image differ in size")
        cap = rows * cols if cap is None else int(cap)
        K4 = np.ascontiguousarray(K4, np.float64).reshape(4); Rinv = np.ascontiguousarray(Rinv, np.float64).reshape(9); c = np.ascontiguousarray(c, np.float64).reshape(3)
        xyz = np.empty((max(cap, 1), 3), np.float64); bgr = np.empty((max(cap, 1), 3), np.uint8); n = C.c_int32(0)
        self._check(self.lib.sfmhip_depth_to_points(self.h, depth.ctypes.data, keep.ctypes.data, ptr, rows, cols, ch, ld, K4.ctypes.data, Rinv.ctypes.data,
                                                    c.ctypes.data, xyz.ctypes.data, bgr.ctypes.data, cap, C.byref(n)))
        m = min(n.value, cap)
        return xyz[:m].copy(), bgr[:m].copy(), n.value

    def depth_to_points_dev(self, d_depth, d_keep, d_img, rows, cols, channels, ld, K4, Rinv, c, d_xyz, d_bgr, cap, d_n_found):
        """the same on resident arrays (K4, Rinv, c stay host arrays); the int32 at d_n_found receives the full count: enqueues only"""
        K4 = np.ascontiguousarray(K4, np.float64).reshape(4); Rinv = np.ascontiguousarray(Rinv, np.float64).reshape(9); c = np.ascontiguousarray(c, np.float64).reshape(3)
        self._check(self.lib.sfmhip_depth_to_points_dev(self.h, _dptr(d_depth), _dptr(d_keep), _dptr(d_img), int(rows), int(cols), int(channels), int(ld),
                                                        K4.ctypes.data, Rinv.ctypes.data, c.ctypes.data, _dptr(d_xyz), _dptr(d_bgr), int(cap), _dptr(d_n_found)))

    # ---------------------------------------------------------------- dense mesh (sfmhip_tsdf_integrate, sfmhip_tsdf_mesh)
    def tsdf_integrate(self, dims, origin, voxel, trunc, depths, keeps, images, K4, R, t, dsum, wsum, csum=None):
        """sfmhip_tsdf_integrate: adds up to 8 views to the caller's volume IN PLACE (dsum, wsum: contiguous int32 arrays of nx*ny*nz
        entries, x fastest; csum: uint32 nvox x 3 with images, None without).  depths: float32 rows x cols maps; keeps: None, or a list
        of uint8 maps / None per view; images: None, or the views' uint8 images (gray or BGR); R (n x 9, world to camera), t (n x 3)"""
        n = len(depths)
        maps = [np.ascontiguousarray(d, np.float32) for d in depths]
        rows, cols = maps[0].shape
        kp = [None if keeps is None or k is None else np.ascontiguousarray(k, np.uint8) for k in (keeps if keeps is not None else [None] * n)]
        if any(m.shape != (rows, cols) for m in maps) or len(kp) != n or any(k is not None and k.shape != (rows, cols) for k in kp):
            raise ValueError("the depth and keep maps differ in size or number")
        ch, ld, img_p = 1, cols, None
        if images is not None:
            ims, ptrs, irows, icols, ch, ld = _dense_images(images)
            if (irows, icols) != (rows, cols) or len(ims) != n:
                raise ValueError("the images and the depth maps differ in size or number")
            img_p = (C.c_void_p * n)(*ptrs)
        _tsdf_volume_ok(dims, dsum, wsum, csum)
        dims_a, origin_a, K4, R, t = _tsdf_host_args(dims, origin, K4, R, t, n)
        depth_p = (C.c_void_p * n)(*[m.ctypes.data for m in maps])
        keep_p = None if keeps is None else (C.c_void_p * n)(*[None if k is None else k.ctypes.data for k in kp])
        self._check(self.lib.sfmhip_tsdf_integrate(self.h, dims_a.ctypes.data, origin_a.ctypes.data, float(voxel), float(trunc), depth_p, keep_p, img_p, n, rows, cols, ch, ld,
                                                   K4.ctypes.data, R.ctypes.data, t.ctypes.data, dsum.ctypes.data, wsum.ctypes.data,
                                                   None if csum is None else csum.ctypes.data))

    def tsdf_integrate_dev(self, dims, origin, voxel, trunc, d_depths, d_keeps, d_images, rows, cols, channels, ld, K4, R, t, d_dsum, d_wsum, d_csum):
        """the same on resident maps, images and volume (torch CUDA tensors or device addresses; d_keeps, or entries of it, and d_images /
        d_csum may be None): enqueues on the context's stream, never synchronises"""
        n = len(d_depths)
        dims_a, origin_a, K4, R, t = _tsdf_host_args(dims, origin, K4, R, t, n)
        depth_p = (C.c_void_p * n)(*[_dptr(x) for x in d_depths])
        keep_p = None if d_keeps is None else (C.c_void_p * n)(*[None if k is None else _dptr(k) for k in d_keeps])
        img_p = None if d_images is None else (C.c_void_p * n)(*[_dptr(x) for x in d_images])
        self._check(self.lib.sfmhip_tsdf_integrate_dev(self.h, dims_a.ctypes.data, origin_a.ctypes.data, float(voxel), float(trunc), depth_p, keep_p, img_p, n, int(rows),
                                                       int(cols), int(channels), int(ld), K4.ctypes.data, R.ctypes.data, t.ctypes.data, _dptr(d_dsum), _dptr(d_wsum),
                                                       None if d_csum is None else _dptr(d_csum)))

    def tsdf_mesh(self, dims, origin, voxel, dsum, wsum, csum=None, min_weight=1, vertex_cap=None, triangle_cap=None):
        """(xyz m x 3 float64, bgr m x 3 uint8 or None without csum, tri k x 3 int32, n_vertices, n_triangles): sfmhip_tsdf_mesh, marching
        tetrahedra on the volume.  Without caps the call is made twice, the first time with caps of 0 for the counts; with caps,
        m = min(n_vertices, vertex_cap) and k = min(n_triangles, triangle_cap)"""
        dsum = np.ascontiguousarray(dsum, np.int32); wsum = np.ascontiguousarray(wsum, np.int32)
        csum = None if csum is None else np.ascontiguousarray(csum, np.uint32)
        _tsdf_volume_ok(dims, dsum, wsum, csum)
        dims_a, origin_a, *_ = _tsdf_host_args(dims, origin, np.zeros(4), np.zeros(9), np.zeros(3), 1)
        nv, nt = C.c_int32(0), C.c_int32(0)

        def call(xyz, bgr, vcap, tri, tcap):
            self._check(self.lib.sfmhip_tsdf_mesh(self.h, dims_a.ctypes.data, origin_a.ctypes.data, float(voxel), dsum.ctypes.data, wsum.ctypes.data,
                                                  None if csum is None else csum.ctypes.data, int(min_weight), None if xyz is None else xyz.ctypes.data,
                                                  None if bgr is None else bgr.ctypes.data, vcap, None if tri is None else tri.ctypes.data, tcap, C.byref(nv), C.byref(nt)))
        if vertex_cap is None or triangle_cap is None:
            call(None, None, 0, None, 0)
            vertex_cap = nv.value if vertex_cap is None else int(vertex_cap)
            triangle_cap = nt.value if triangle_cap is None else int(triangle_cap)
        vcap, tcap = int(vertex_cap), int(triangle_cap)
        xyz = np.empty((max(vcap, 1), 3), np.float64); tri = np.empty((max(tcap, 1), 3), np.int32)
        bgr = None if csum is None else np.empty((max(vcap, 1), 3), np.uint8)
        call(xyz, bgr, vcap, tri, tcap)
        m, k = min(nv.value, vcap), min(nt.value, tcap)
        return xyz[:m].copy(), None if bgr is None else bgr[:m].copy(), tri[:k].copy(), nv.value, nt.value

    def tsdf_mesh_dev(self, dims, origin, voxel, d_dsum, d_wsum, d_csum, min_weight, d_xyz, d_bgr, vertex_cap, d_tri, triangle_cap, d_n_vertices, d_n_triangles):
        """the same on a resident volume into resident arrays (any of d_csum, d_xyz, d_bgr, d_tri may be None); the int32s at d_n_vertices and
        d_n_triangles receive the full counts: enqueues only"""
        dims_a, origin_a, *_ = _tsdf_host_args(dims, origin, np.zeros(4), np.zeros(9), np.zeros(3), 1)

        def p(x):
            return None if x is None else _dptr(x)
        self._check(self.lib.sfmhip_tsdf_mesh_dev(self.h, dims_a.ctypes.data, origin_a.ctypes.data, float(voxel), _dptr(d_dsum), _dptr(d_wsum), p(d_csum), int(min_weight),
                                                  p(d_xyz), p(d_bgr), int(vertex_cap), p(d_tri), int(triangle_cap), _dptr(d_n_vertices), _dptr(d_n_triangles)))

    # ---------------------------------------------------------------- mesh clean-up (sfmhip_mesh_*)
    @staticmethod
    def _mesh_arrays(xyz, bgr, tri):
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3); tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
        if bgr is not None:
            bgr = np.ascontiguousarray(bgr, np.uint8).reshape(-1, 3)
            if len(bgr) != len(xyz):
                raise ValueError("one colour per vertex")
        return xyz, bgr, tri

    def mesh_components(self, nv, tri):
        """(tri_label int32 nt, vertex_label int32 nv, sizes int32 C): the connected components of a triangle mesh, two triangles connected
        when they share a vertex, numbered by their smallest vertex (sfmhip_mesh_components); -1 for an invalid triangle and for an
        unreferenced vertex"""
        tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
        nv, nt = int(nv), len(tri)
        tl = np.full(nt, -1, np.int32); vl = np.full(nv, -1, np.int32); sizes = np.zeros(nt, np.int32); m = C.c_int(0)
        self._check(self.lib.sfmhip_mesh_components(self.h, nv, tri.ctypes.data, nt, tl.ctypes.data, vl.ctypes.data, C.byref(m), sizes.ctypes.data))
        return tl, vl, sizes[:m.value].copy()

    def mesh_components_dev(self, nv, d_tri, nt, d_tri_label, d_vertex_label, d_n_components, d_sizes=None):
        """the same on resident arrays (d_vertex_label / d_sizes may be None); d_sizes holds nt entries, zero from the number of components
        on: enqueues only"""
        self._check(self.lib.sfmhip_mesh_components_dev(self.h, int(nv), _dptr(d_tri), int(nt), _dptr(d_tri_label), _dptr(d_vertex_label), _dptr(d_n_components),
                                                        _dptr(d_sizes)))

    def _mesh_rebuild(self, fn, xyz, bgr, tri, *params):
        xyz, bgr, tri = self._mesh_arrays(xyz, bgr, tri)
        nv, nt = len(xyz), len(tri)
        xo = np.empty((nv, 3), np.float64); bo = None if bgr is None else np.empty((nv, 3), np.uint8); to = np.empty((nt, 3), np.int32)
        vmap = np.full(nv, -1, np.int32); m, k = C.c_int(0), C.c_int(0)
        self._check(fn(self.h, xyz.ctypes.data, None if bgr is None else bgr.ctypes.data, nv, tri.ctypes.data, nt, *params, xo.ctypes.data,
                       None if bo is None else bo.ctypes.data, to.ctypes.data, vmap.ctypes.data, C.byref(m), C.byref(k)))
        return xo[:m.value].copy(), None if bo is None else bo[:m.value].copy(), to[:k.value].copy(), vmap

    def mesh_filter_components(self, xyz, bgr, tri, min_triangles=1, keep_largest=False):
        """(xyz, bgr or None, tri, vertex_map): the components with at least min_triangles triangles, or of those only the largest (the
        smallest number among equals); the kept triangles in their order, the vertices they name in theirs (sfmhip_mesh_filter_components).
        The defaults drop invalid triangles and unreferenced vertices and nothing else."""
        return self._mesh_rebuild(self.lib.sfmhip_mesh_filter_components, xyz, bgr, tri, int(min_triangles), int(bool(keep_largest)))

    def mesh_filter_components_dev(self, d_xyz, d_bgr, nv, d_tri, nt, min_triangles, keep_largest, d_xyz_out, d_bgr_out, d_tri_out, d_vertex_map, d_nv_out, d_nt_out):
        """the same on resident arrays (d_bgr with d_bgr_out, and d_vertex_map, may be None); outputs of nv / nt rows, the int32s at d_nv_out /
        d_nt_out receive the counts: enqueues only"""
        self._check(self.lib.sfmhip_mesh_filter_components_dev(self.h, _dptr(d_xyz), _dptr(d_bgr), int(nv), _dptr(d_tri), int(nt), int(min_triangles),
                                                               int(bool(keep_largest)), _dptr(d_xyz_out), _dptr(d_bgr_out), _dptr(d_tri_out), _dptr(d_vertex_map),
                                                               _dptr(d_nv_out), _dptr(d_nt_out)))

    def mesh_simplify(self, xyz, bgr, tri, voxel):
        """(xyz, bgr or None, tri, vertex_map): vertex clustering on cells of edge `voxel` -- the centroids of sfmhip_voxel_downsample over
        the referenced vertices, the distinct non-degenerate triangles between them in ascending order (sfmhip_mesh_simplify)"""
        return self._mesh_rebuild(self.lib.sfmhip_mesh_simplify, xyz, bgr, tri, float(voxel))

    def mesh_simplify_dev(self, d_xyz, d_bgr, nv, d_tri, nt, voxel, d_xyz_out, d_bgr_out, d_tri_out, d_vertex_map, d_nv_out, d_nt_out):
        """the same on resident arrays; the int32 at d_nv_out becomes -1 where the cell is too small for the mesh's extent: enqueues only"""
        self._check(self.lib.sfmhip_mesh_simplify_dev(self.h, _dptr(d_xyz), _dptr(d_bgr), int(nv), _dptr(d_tri), int(nt), float(voxel), _dptr(d_xyz_out), _dptr(d_bgr_out),
                                                      _dptr(d_tri_out), _dptr(d_vertex_map), _dptr(d_nv_out), _dptr(d_nt_out)))

    def mesh_vertex_normals(self, xyz, tri):
        """nv x 3 float64: area-weighted unit normals, zeros where there is none (sfmhip_mesh_vertex_normals)"""
        xyz, _, tri = self._mesh_arrays(xyz, None, tri)
        out = np.zeros((len(xyz), 3), np.float64)
        self._check(self.lib.sfmhip_mesh_vertex_normals(self.h, xyz.ctypes.data, len(xyz), tri.ctypes.data, len(tri), out.ctypes.data))
        return out

    def mesh_vertex_normals_dev(self, d_xyz, nv, d_tri, nt, d_normals):
        self._check(self.lib.sfmhip_mesh_vertex_normals_dev(self.h, _dptr(d_xyz), int(nv), _dptr(d_tri), int(nt), _dptr(d_normals)))

    def mesh_smooth(self, xyz, tri, iterations=10, lam=0.5, mu=-0.53):
        """nv x 3 float64: `iterations` Taubin pairs of steps (lam, then mu), or Laplacian steps with lam where mu == 0
        (sfmhip_mesh_smooth); no boundary pinning"""
        xyz, _, tri = self._mesh_arrays(xyz, None, tri)
        out = np.empty((len(xyz), 3), np.float64)
        self._check(self.lib.sfmhip_mesh_smooth(self.h, xyz.ctypes.data, len(xyz), tri.ctypes.data, len(tri), int(iterations), float(lam), float(mu), out.ctypes.data))
        return out

    def mesh_smooth_dev(self, d_xyz, nv, d_tri, nt, iterations, lam, mu, d_xyz_out):
        self._check(self.lib.sfmhip_mesh_smooth_dev(self.h, _dptr(d_xyz), int(nv), _dptr(d_tri), int(nt), int(iterations), float(lam), float(mu), _dptr(d_xyz_out)))

    # ---------------------------------------------------------------- semi-global aggregation of the sweep's costs (sfmhip_sgm_depth)
    def sweep_costs(self, ref, srcs, A, b, planes, wmin, wmax, radius=2, min_sources=1, cost_scale=262144.0):
        """rows x cols x planes uint16: sfmhip_sweep_costs, the sweep's plane scores as costs (65535 = not scored)"""
        imgs, ptrs, rows, cols, ch, ld = _dense_images([ref] + list(srcs))
        n = len(imgs) - 1
        A = np.ascontiguousarray(A, np.float32).reshape(n, 9); b = np.ascontiguousarray(b, np.float32).reshape(n, 3)
        cost = np.empty((rows, cols, max(int(planes), 1)), np.uint16)
        src = (C.c_void_p * max(n, 1))(*ptrs[1:])
        self._check(self.lib.sfmhip_sweep_costs(self.h, ptrs[0], src, n, rows, cols, ch, ld, A.ctypes.data, b.ctypes.data, int(planes), float(wmin), float(wmax),
                                                int(radius), int(min_sources), float(cost_scale), cost.ctypes.data))
        return cost

    def sweep_costs_dev(self, d_ref, d_srcs, rows, cols, channels, ld, A, b, planes, wmin, wmax, radius, min_sources, cost_scale, d_cost):
        """the same on resident images into a resident volume (A and b stay host arrays): enqueues only"""
        n = len(d_srcs)
        A = np.ascontiguousarray(A, np.float32).reshape(n, 9); b = np.ascontiguousarray(b, np.float32).reshape(n, 3)
        src = (C.c_void_p * max(n, 1))(*[_dptr(x) for x in d_srcs])
        self._check(self.lib.sfmhip_sweep_costs_dev(self.h, _dptr(d_ref), src, n, int(rows), int(cols), int(channels), int(ld), A.ctypes.data, b.ctypes.data,
                                                    int(planes), float(wmin), float(wmax), int(radius), int(min_sources), float(cost_scale), _dptr(d_cost)))

    def sgm_depth(self, cost, wmin, wmax, P1, P2, paths=8, max_cost=65535, return_sums=False):
        """(plane int32, cost uint16, sum uint32, depth float32), each rows x cols: sfmhip_sgm_depth of a rows x cols x planes uint16 cost
        volume; return_sums: also S (rows x cols x planes uint32), the aggregated volume"""
        cost = np.ascontiguousarray(cost, np.uint16)
        rows, cols, D = cost.shape
        plane = np.empty((rows, cols), np.int32); wc = np.empty((rows, cols), np.uint16); ssum = np.empty((rows, cols), np.uint32)
        depth = np.empty((rows, cols), np.float32)
        S = np.empty((rows, cols, D), np.uint32) if return_sums else None
        self._check(self.lib.sfmhip_sgm_depth(self.h, cost.ctypes.data, rows, cols, D, float(wmin), float(wmax), int(P1), int(P2), int(paths), int(max_cost),
                                              plane.ctypes.data, wc.ctypes.data, ssum.ctypes.data, depth.ctypes.data, S.ctypes.data if return_sums else None))
        return (plane, wc, ssum, depth, S) if return_sums else (plane, wc, ssum, depth)

    def sgm_depth_dev(self, d_cost, rows, cols, planes, wmin, wmax, P1, P2, paths, max_cost, d_plane, d_win_cost, d_sum, d_depth, d_S=None):
        """the same on a resident volume; any output may be None but not all of the first four: enqueues only"""
        self._check(self.lib.sfmhip_sgm_depth_dev(self.h, _dptr(d_cost), int(rows), int(cols), int(planes), float(wmin), float(wmax), int(P1), int(P2), int(paths),
                                                  int(max_cost), _dptr(d_plane), _dptr(d_win_cost), _dptr(d_sum), _dptr(d_depth), _dptr(d_S)))

    def plane_sweep_sgm(self, ref, srcs, A, b, planes, wmin, wmax, radius=2, min_sources=1, cost_scale=262144.0, P1=512, P2=4096, paths=8, max_cost=65535):
        """(plane int32, cost uint16, depth float32), each rows x cols: sfmhip_plane_sweep_sgm, the sweep's costs aggregated along 4 or 8
        directions before the winner is taken; the volumes stay on the device"""
        imgs, ptrs, rows, cols, ch, ld = _dense_images([ref] + list(srcs))
        n = len(imgs) - 1
        A = np.ascontiguousarray(A, np.float32).reshape(n, 9); b = np.ascontiguousarray(b, np.float32).reshape(n, 3)
        plane = np.empty((rows, cols), np.int32); wc = np.empty((rows, cols), np.uint16); depth = np.empty((rows, cols), np.float32)
        src = (C.c_void_p * max(n, 1))(*ptrs[1:])
        self._check(self.lib.sfmhip_plane_sweep_sgm(self.h, ptrs[0], src, n, rows, cols, ch, ld, A.ctypes.data, b.ctypes.data, int(planes), float(wmin), float(wmax),
                                                    int(radius), int(min_sources), float(cost_scale), int(P1), int(P2), int(paths), int(max_cost), plane.ctypes.data,
                                                    wc.ctypes.data, depth.ctypes.data))
        return plane, wc, depth

    def plane_sweep_sgm_dev(self, d_ref, d_srcs, rows, cols, channels, ld, A, b, planes, wmin, wmax, radius, min_sources, cost_scale, P1, P2, paths, max_cost,
                            d_plane, d_win_cost, d_depth):
        """the same on resident images: enqueues only"""
        n = len(d_srcs)
        A = np.ascontiguousarray(A, np.float32).reshape(n, 9); b = np.ascontiguousarray(b, np.float32).reshape(n, 3)
        src = (C.c_void_p * max(n, 1))(*[_dptr(x) for x in d_srcs])
        self._check(self.lib.sfmhip_plane_sweep_sgm_dev(self.h, _dptr(d_ref), src, n, int(rows), int(cols), int(channels), int(ld), A.ctypes.data, b.ctypes.data,
                                                        int(planes), float(wmin), float(wmax), int(radius), int(min_sources), float(cost_scale), int(P1), int(P2),
                                                        int(paths), int(max_cost), _dptr(d_plane), _dptr(d_win_cost), _dptr(d_depth)))

    def select_views(self, ext, pts, obs_cam, obs_pt, n_src=2, min_angle_deg=1.0):
        """SelectedViews of sfmhip_select_views (where the definition is): the covisibility counts of the views, every view's n_src sources
        ranked by the sparse points shared under at least min_angle_deg, and every view's inverse-depth range from the points it sees.
        ext: the bundle adjustment's (angle-axis, t) rows; pts n x 3; obs_cam, obs_pt: its observation lists"""
        ext = np.ascontiguousarray(ext, np.float64).reshape(-1, 6); pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        oc = np.ascontiguousarray(obs_cam, np.int32).ravel(); op = np.ascontiguousarray(obs_pt, np.int32).ravel()
        if len(oc) != len(op):
            raise ValueError("obs_cam and obs_pt are lists of one length")
        n, k = len(ext), int(n_src)
        shared = np.zeros((n, n), np.int32); score = np.zeros((n, n), np.int32); sources = np.zeros((n, max(k, 0)), np.int32); n_scored = np.zeros(n, np.int32)
        wrange = np.zeros((n, 2)); n_depth = np.zeros(n, np.int32)
        self._check(self.lib.sfmhip_select_views(self.h, ext.ctypes.data, n, pts.ctypes.data if len(pts) else None, len(pts), oc.ctypes.data if len(oc) else None,
                                                 op.ctypes.data if len(op) else None, len(oc), select_cos2(min_angle_deg), k, shared.ctypes.data, score.ctypes.data,
                                                 sources.ctypes.data, n_scored.ctypes.data, wrange.ctypes.data, n_depth.ctypes.data))
        return SelectedViews(shared, score, sources, n_scored, wrange, n_depth)

    def select_views_dev(self, ext, d_pts, n_pt, d_obs_cam, d_obs_pt, n_obs, n_src, min_angle_deg, d_shared=None, d_score=None, d_sources=None, d_n_scored=None,
                         d_wrange=None, d_n_depth=None):
        """the same on resident arrays (torch CUDA tensors or device addresses; ext stays a host array), any output may be None: enqueues
        on the context's stream, never synchronises.  An observation with an index out of range is ignored"""
        ext = np.ascontiguousarray(ext, np.float64).reshape(-1, 6)
        self._check(self.lib.sfmhip_select_views_dev(self.h, ext.ctypes.data, len(ext), _dptr(d_pts), int(n_pt), _dptr(d_obs_cam), _dptr(d_obs_pt), int(n_obs),
                                                     select_cos2(min_angle_deg), int(n_src), _dptr(d_shared), _dptr(d_score), _dptr(d_sources), _dptr(d_n_scored),
                                                     _dptr(d_wrange), _dptr(d_n_depth)))

    # ---------------------------------------------------------------- tracks from pairwise matches
    def build_tracks(self, n_kp, pairs, matches, counts, kp=None, min_len=2, conflicts="drop", filter_matches=True):
        """Tracks of sfmhip_build_tracks (where the definition is) from match lists of any pair list.  n_kp: key points per image; pairs
        (n_pairs, 2); matches (n_pairs, max_per_pair) DMATCH and counts (n_pairs,), the layout match_pairs_dev leaves; kp: one KEYPOINT
        array per image, for obs_uv.  Returns (track_of, obs_cam, obs_pt, obs_kp, obs_uv or None, track_len, stats, matches_out,
        counts_out), trimmed to the written prefixes (matches_out: full rows, counts_out[q] of them written; both None without
        filter_matches)"""
        n_kp = np.ascontiguousarray(n_kp, np.int32).ravel(); pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        matches = np.ascontiguousarray(matches, DMATCH); counts = np.ascontiguousarray(counts, np.int32).ravel()
        flags = _tracks_flags(min_len, conflicts)
        P = len(pairs)
        if matches.ndim != 2 or matches.shape[0] != P or len(counts) != P:
            raise ValueError("matches is n_pairs x max_per_pair, counts n_pairs")
        if (n_kp < 0).any() or int(n_kp.astype(np.int64).sum()) >= 2 ** 31:
            raise ValueError("n_kp: non-negative counts with a sum below 2^31")
        n = int(n_kp.sum()); S = matches.shape[1]
        arr = None
        if kp is not None:
            if len(kp) != len(n_kp):
                raise ValueError("one key-point array per image")
            kp = [np.ascontiguousarray(k, KEYPOINT) for k in kp]
            if any(len(k) < c for k, c in zip(kp, n_kp)):
                raise ValueError("a key-point array is shorter than n_kp says")
            arr = (C.c_void_p * len(kp))(*[k.ctypes.data if len(k) else None for k in kp])
        track_of = np.empty(n, np.int32); oc = np.empty(n, np.int32); op = np.empty(n, np.int32); ok = np.empty(n, np.int32)
        uv = np.empty((n, 2)) if kp is not None else None
        tl = np.empty(n // 2, np.int32); stats = np.zeros(8, np.int32)
        mo = np.zeros((P, S), DMATCH) if filter_matches else None
        co = np.zeros(P, np.int32) if filter_matches else None
        self._check(self.lib.sfmhip_build_tracks(self.h, len(n_kp), n_kp.ctypes.data, pairs.ctypes.data if P else None, P, matches.ctypes.data if P * S else None, S,
                                                 counts.ctypes.data if P else None, arr, int(min_len), flags, _ptr(track_of), _ptr(oc), _ptr(op), _ptr(ok), _ptr(uv),
                                                 _ptr(tl), _ptr(mo), _ptr(co), _ptr(stats)))
        nt, no = int(stats[0]), int(stats[1])
        return track_of, oc[:no], op[:no], ok[:no], (uv[:no] if uv is not None else None), tl[:nt], stats, mo, co

    def build_tracks_dev(self, n_kp, pairs, d_matches, max_per_pair, d_counts, d_kp=None, min_len=2, conflicts="drop", d_track_of=None, d_obs_cam=None,
                         d_obs_pt=None, d_obs_kp=None, d_obs_uv=None, d_track_len=None, d_matches_out=None, d_counts_out=None, d_stats=None):
        """the same on resident arrays (torch CUDA tensors or device addresses; n_kp and pairs stay host arrays, d_kp is a list of
        device KEYPOINT arrays), any output may be None: enqueues on the context's stream, never synchronises.  d_stats[0] = -1: a
        union gave up"""
        n_kp = np.ascontiguousarray(n_kp, np.int32).ravel(); pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        flags = _tracks_flags(min_len, conflicts)
        arr = None
        if d_kp is not None:
            if len(d_kp) != len(n_kp):
                raise ValueError("one key-point array per image")
            arr = (C.c_void_p * len(d_kp))(*[_dptr(k) for k in d_kp])
        self._check(self.lib.sfmhip_build_tracks_dev(self.h, len(n_kp), n_kp.ctypes.data, pairs.ctypes.data if len(pairs) else None, len(pairs), _dptr(d_matches),
                                                     int(max_per_pair), _dptr(d_counts), arr, int(min_len), flags, _dptr(d_track_of), _dptr(d_obs_cam),
                                                     _dptr(d_obs_pt), _dptr(d_obs_kp), _dptr(d_obs_uv), _dptr(d_track_len), _dptr(d_matches_out),
                                                     _dptr(d_counts_out), _dptr(d_stats)))

    def points_fallback_count(self):
        """queries the last grid search of this context handed to its brute-force pass (synchronises)"""
        c = C.c_int(0)
        self._check(self.lib.sfmhip_points_fallback_count(self.h, C.byref(c)))
        return c.value


def _jpeg_bytes(data):
    """a contiguous uint8 array over a file's bytes (bytes / bytearray / memoryview, or a uint8 array)"""
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8:
            raise ValueError("a JPEG file is bytes or a uint8 array")
        return np.ascontiguousarray(data).reshape(-1)
    return np.frombuffer(data, np.uint8)


def jpeg_info(data):
    """(rows, cols, channels, restart_interval, n_intervals) from the headers of a baseline JPEG file's bytes (sfmhip_jpeg_info: host
    only, no context).  SfmHipError for a file the decoder refuses."""
    buf = _jpeg_bytes(data)
    v = [C.c_int(0) for _ in range(5)]
    rc = _lib.load().sfmhip_jpeg_info(buf.ctypes.data if buf.size else None, buf.size, *[C.byref(x) for x in v])
    if rc != 0:
        raise SfmHipError(f"libsfmhip error {rc}: not a baseline JPEG the decoder supports, or damaged headers")
    return tuple(x.value for x in v)


def _const_mask(m, n):
    """None, or a contiguous uint8 array of n flags (bool / integer input)"""
    if m is None:
        return None
    a = np.ascontiguousarray(np.asarray(m).reshape(-1) != 0, np.uint8)
    if a.shape[0] != n:
        raise ValueError(f"constant mask of {a.shape[0]} entries for {n} blocks")
    return a


def _mask_ptr(a):
    return None if a is None else a.ctypes.data


def _index_mask(idx, n):
    """index list -> uint8 flags (None stays None)"""
    if idx is None:
        return None
    idx = np.asarray(idx, np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise ValueError("constant block index out of range")
    m = np.zeros(n, np.uint8); m[idx] = 1
    return m


class BAProblem:
    """HBM-resident BA problem (sfmhip_ba_create; with cam_const / pt_const: sfmhip_ba_create_ex)."""

    def __init__(self, ctx, K4, ext, pts, obs_cam, obs_pt, obs_uv, opts=None, cam_const=None, pt_const=None):
        self.ctx = ctx
        K4 = np.ascontiguousarray(K4, np.float64).reshape(4); ext = np.ascontiguousarray(ext, np.float64).reshape(-1, 6)
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        oc = np.ascontiguousarray(obs_cam, np.int32); op = np.ascontiguousarray(obs_pt, np.int32)
        uv = np.ascontiguousarray(obs_uv, np.float64).reshape(-1, 2)
        self.n_cam, self.n_pt, self.n_obs = ext.shape[0], pts.shape[0], oc.shape[0]
        o = opts if opts is not None else ctx.ba_options()
        self.opts = o
        h = C.c_void_p()
        if cam_const is None and pt_const is None:
            ctx._check(ctx.lib.sfmhip_ba_create(ctx.h, K4.ctypes.data, ext.ctypes.data, self.n_cam, pts.ctypes.data, self.n_pt,
                                                oc.ctypes.data, op.ctypes.data, uv.ctypes.data, self.n_obs, C.byref(o), C.byref(h)))
        else:
            cm, pm = _const_mask(cam_const, self.n_cam), _const_mask(pt_const, self.n_pt)
            ctx._check(ctx.lib.sfmhip_ba_create_ex(ctx.h, K4.ctypes.data, ext.ctypes.data, self.n_cam, pts.ctypes.data, self.n_pt,
                                                   oc.ctypes.data, op.ctypes.data, uv.ctypes.data, self.n_obs, _mask_ptr(cm), _mask_ptr(pm),
                                                   C.byref(o), C.byref(h)))
        self.h = h
        self._cb = None

    def set_allreduce(self, fn, rank, world):
        """fn(dev_ptr:int, count:int, stream:int) -> 0 on success; sums `count` doubles in place over all ranks."""
        def _tramp(user, buf, count, stream):
            try:
                return int(fn(buf, count, stream) or 0)
            except Exception:   # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return -1
        self._cb = _lib.ALLREDUCE_FN(_tramp)
        self.ctx._check(self.ctx.lib.sfmhip_ba_set_allreduce(self.h, self._cb, None, int(rank), int(world)))

    def set_rccl(self, comm, rank, world):
        """install the in-library RCCL hook (sfmhip_ba_set_rccl); comm from Context.rccl_comm_create"""
        self._cb = None
        self.ctx._check(self.ctx.lib.sfmhip_ba_set_rccl(self.h, comm, int(rank), int(world)))

    def run(self):
        s = BASummary()
        self.ctx._check(self.ctx.lib.sfmhip_ba_run(self.h, C.byref(s)))
        return s.asdict()

    def iterate(self, n):
        s = BASummary()
        self.ctx._check(self.ctx.lib.sfmhip_ba_iterate(self.h, int(n), C.byref(s)))
        return s.asdict()

    def reset(self):
        self.ctx._check(self.ctx.lib.sfmhip_ba_reset(self.h))

    def params(self):
        K4 = np.empty(4); ext = np.empty((self.n_cam, 6)); pts = np.empty((self.n_pt, 3))
        self.ctx._check(self.ctx.lib.sfmhip_ba_get_params(self.h, K4.ctypes.data, ext.ctypes.data, pts.ctypes.data))
        return K4, ext, pts

    def reduced_system(self, radius):
        n = C.c_int(); cost = C.c_double()
        self.ctx._check(self.ctx.lib.sfmhip_ba_reduced_system(self.h, radius, None, None, C.byref(n), C.byref(cost)))
        S = np.zeros((n.value, n.value)); rhs = np.zeros(n.value)
        self.ctx._check(self.ctx.lib.sfmhip_ba_reduced_system(self.h, radius, S.ctypes.data, rhs.ctypes.data, C.byref(n), C.byref(cost)))
        return S, rhs, cost.value

    _TABLE_DTYPES = {"ouv": np.float64, "cam_uv": np.float64, "setup_ms": np.float64, "step_scalars": np.float64}

    def debug_table(self, name):
        """One of the tables sfmhip_ba_create built on the device (sfmhip_ba_debug_table), as a numpy array."""
        nb = C.c_size_t()
        self.ctx._check(self.ctx.lib.sfmhip_ba_debug_table(self.h, name.encode(), None, 0, C.byref(nb)))
        dt = np.dtype(self._TABLE_DTYPES.get(name, np.int32))
        out = np.empty(nb.value // dt.itemsize, dt)
        self.ctx._check(self.ctx.lib.sfmhip_ba_debug_table(self.h, name.encode(), out.ctypes.data, out.nbytes, C.byref(nb)))
        return out

    def phase_ms(self):
        out = (C.c_double * 8)()
        self.ctx._check(self.ctx.lib.sfmhip_ba_phase_ms(self.h, out))
        return list(out)

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.lib.sfmhip_ba_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ba_solve_multi(ctxs, K4, ext, pts, obs_cam, obs_pt, obs_uv, opts=None, cam_const=None, pt_const=None):
    """sfmhip_ba_solve_multi on copies: one context per GPU of this process (two contexts on one device: host-staged rehearsal).
    cam_const / pt_const: as Context.ba_create (sfmhip_ba_solve_multi_ex).  Returns (K4, ext, pts, summary dict)."""
    K4 = np.array(K4, np.float64).reshape(4).copy(); ext = np.array(ext, np.float64).reshape(-1, 6).copy()
    pts = np.array(pts, np.float64).reshape(-1, 3).copy()
    oc = np.ascontiguousarray(obs_cam, np.int32); op = np.ascontiguousarray(obs_pt, np.int32)
    uv = np.ascontiguousarray(obs_uv, np.float64).reshape(-1, 2)
    o = opts if opts is not None else ctxs[0].ba_options()
    s = BASummary()
    arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
    if cam_const is None and pt_const is None:
        ctxs[0]._check(ctxs[0].lib.sfmhip_ba_solve_multi(arr, len(ctxs), K4.ctypes.data, ext.ctypes.data, ext.shape[0], pts.ctypes.data, pts.shape[0],
                                                          oc.ctypes.data, op.ctypes.data, uv.ctypes.data, oc.shape[0], C.byref(o), C.byref(s)))
    else:
        cm, pm = _const_mask(cam_const, ext.shape[0]), _const_mask(pt_const, pts.shape[0])
        ctxs[0]._check(ctxs[0].lib.sfmhip_ba_solve_multi_ex(arr, len(ctxs), K4.ctypes.data, ext.ctypes.data, ext.shape[0], pts.ctypes.data,
                                                             pts.shape[0], oc.ctypes.data, op.ctypes.data, uv.ctypes.data, oc.shape[0],
                                                             _mask_ptr(cm), _mask_ptr(pm), C.byref(o), C.byref(s)))
    return K4, ext, pts, s.asdict()


def match_pairs_multi(ctxs, mats, pairs, ratio=0.6, floor_=10.0, mult=5.0, cross_check=False):
    """sfmhip_match_pairs_multi: host matrices (float32: L2, uint8: Hamming2) matched over several contexts of this process, the pairs in
    contiguous blocks; list of DMATCH arrays in pair order."""
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    n_pairs, n = pairs.shape[0], len(mats)
    if n_pairs == 0:
        return []
    ham = np.asarray(mats[0]).dtype == np.uint8
    arrs = [np.ascontiguousarray(m, np.uint8 if ham else np.float32) for m in mats]
    dim = arrs[0].shape[1]
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    rows = np.array([a.shape[0] for a in arrs], np.int32)
    mpp = max(1, int(rows[pairs[:, 0]].max()))
    out = np.empty((n_pairs, mpp), DMATCH); counts = np.zeros(n_pairs, np.int32)
    carr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
    ctxs[0]._check(ctxs[0].lib.sfmhip_match_pairs_multi_ex(carr, len(ctxs), 2 if ham else 1, ptrs, rows.ctypes.data, dim, None, n, pairs.ctypes.data,
                                                            n_pairs, ratio, floor_, mult, _lib.MATCH_MUTUAL if cross_check else 0,
                                                            out.ctypes.data, mpp, counts.ctypes.data))
    return [out[p, :c] for p, c in enumerate(counts.tolist())]


def ratio_filter(idx2, dist2, ratio=0.6, floor_=10.0, mult=5.0):
    """sfmhip_ratio_filter (host C, needs no GPU): the tail of match_features, NViewReconstuct.cpp:880-908."""
    lib = _lib.load()
    idx2 = np.ascontiguousarray(idx2, np.int32); dist2 = np.ascontiguousarray(dist2, np.float32)
    nq = idx2.shape[0]
    out = np.zeros(max(nq, 1), DMATCH); n = C.c_int()
    rc = lib.sfmhip_ratio_filter(idx2.ctypes.data, dist2.ctypes.data, nq, ratio, floor_, mult, out.ctypes.data, C.byref(n))
    if rc != 0:
        raise SfmHipError(f"sfmhip_ratio_filter failed with {rc}")
    return out[:n.value].copy()


# ------------------------------------------------------------------------------------------------
# mirror of the reference's free functions (same names, same argument meaning)
# ------------------------------------------------------------------------------------------------
_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def match_features(query, train, ctx=None, cross_check=False):
    """NViewReconstuct.cpp:873 (uint8 rows -> NORM_HAMMING2) / TwoViewReconstruct.cpp:156 (float32 rows -> NORM_L2).
    Returns the DMatch array in query order.  cross_check=True: only mutual nearest neighbours survive (no reference counterpart)."""
    ctx = ctx or default_context()
    query = np.asarray(query); train = np.asarray(train)
    if query.dtype == np.uint8:
        sets = [ctx.descset_hamming2(query), ctx.descset_hamming2(train)]
    else:
        sets = [ctx.descset_l2(query), ctx.descset_l2(train)]
    if query.shape[0] == 0:
        return np.zeros(0, DMATCH)
    return ctx.match_pairs(sets, [[0, 1]], cross_check=cross_check)[0]


def match_features_for_all(descriptor_for_all, ctx=None, cross_check=False):
    """NViewReconstuct.cpp:850-871: consecutive pairs (i, i+1); one batched launch sequence for the whole chain."""
    ctx = ctx or default_context()
    n = len(descriptor_for_all)
    if n < 2:
        return []
    pairs = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    mats = [np.asarray(d) for d in descriptor_for_all]
    if len({(m.dtype, m.shape[1]) for m in mats}) == 1 and mats[0].dtype in (np.float32, np.uint8):
        # ONE C call for the whole chain (sfmhip_match_pairs_multi on this context: sets created from the host matrices in one pass of
        # the staging threads, one preparation launch, one batched kNN-2 + ratio tail, sets released)
        out = match_pairs_multi([ctx], mats, pairs, cross_check=cross_check)
    else:
        sets = ctx.descsets_host(mats)
        out = ctx.match_pairs(sets, pairs, cross_check=cross_check)
    for i, m in enumerate(out):
        if len(m) == 0:
            print("[Warning]: zero matches between %d and %d." % (i, i + 1))
    return out


def verify_matches_for_all(K, key_points_for_all, matches_for_all, px=1.0, hypotheses=1024, rounds=3, seed=0, min_inliers=15, ctx=None):
    """Geometric verification of the chain's match lists (no reference counterpart: the reference rejects epipolar outliers for its first
    pair only, NViewReconstuct.cpp:1032): matches_for_all[i] joins images i and i + 1, as match_features_for_all returns them.  The key
    points are normalised by K, the threshold is px pixels (t = px / (0.5 (fx + fy))), all pairs run in one call of sfmhip_verify_pairs.
    Returns (filtered lists, [(count, F 3 x 3)] per pair); a pair without a model of min_inliers rows keeps its matches as they are, with
    a warning, count 0 and a NaN F."""
    ctx = ctx or default_context()
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    blocks = []
    for i, m in enumerate(matches_for_all):
        a, b = key_points_for_all[i], key_points_for_all[i + 1]
        q, t = m["queryIdx"], m["trainIdx"]
        blocks.append(np.stack([(a["x"][q].astype(np.float64) - cx) / fx, (a["y"][q].astype(np.float64) - cy) / fy,
                                (b["x"][t].astype(np.float64) - cx) / fx, (b["y"][t].astype(np.float64) - cy) / fy], 1).reshape(-1, 4))
    if not blocks:
        return [], []
    masks, counts, F, _ = ctx.verify_pairs(blocks, px / (0.5 * (fx + fy)), hypotheses, rounds, seed, min_inliers)
    out = []
    for i, m in enumerate(matches_for_all):
        if counts[i] == 0:
            print("[Warning]: pair %d: no epipolar model with %d matches, the %d matches are kept as they are." % (i, min_inliers, len(m)))
            out.append(m)
        else:
            out.append(m[masks[i]])
    return out, [(int(c), f) for c, f in zip(counts, F)]


GEOMETRY_KINDS = ("none", "general", "planar-or-panoramic")      # kind 0, 1, 2 of sfmhip_two_view_geometry


def two_view_geometry_for_all(K, key_points_for_all, matches_for_all, px=1.0, px_h=2.0, hypotheses=1024, rounds=3, seed=0, min_inliers=15,
                              hf_ratio=0.8, ctx=None):
    """verify_matches_for_all with a homography RANSAC beside the epipolar one and the F/H selection of sfmhip_two_view_geometry: the
    thresholds are px pixels for F and px_h pixels for the homography (a transfer distance carries the noise of both images).  Returns
    (kept lists, [(kind, count, cF, cH, F 3 x 3, Hm 3 x 3)] per pair): a pair of kind 1 (general) keeps F's inliers, a pair of kind 2
    (planar or panoramic: its two-view pose is ill-determined, a warning says so) the homography's, and a pair of kind 0 keeps its
    matches as they are, with a warning."""
    ctx = ctx or default_context()
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    blocks = []
    for i, m in enumerate(matches_for_all):
        a, b = key_points_for_all[i], key_points_for_all[i + 1]
        q, t = m["queryIdx"], m["trainIdx"]
        blocks.append(np.stack([(a["x"][q].astype(np.float64) - cx) / fx, (a["y"][q].astype(np.float64) - cy) / fy,
                                (b["x"][t].astype(np.float64) - cx) / fx, (b["y"][t].astype(np.float64) - cy) / fy], 1).reshape(-1, 4))
    if not blocks:
        return [], []
    f = 0.5 * (fx + fy)
    kind, masks, counts, c2, F, Hm, _ = ctx.two_view_geometry(blocks, px / f, px_h / f, hypotheses, rounds, seed, min_inliers, hf_ratio)
    out = []
    for i, m in enumerate(matches_for_all):
        if kind[i] == 0:
            print("[Warning]: pair %d: no two-view model with %d matches, the %d matches are kept as they are." % (i, min_inliers, len(m)))
            out.append(m)
        else:
            if kind[i] == 2:
                print("[Warning]: pair %d: planar or panoramic (H explains %d matches, F %d): its two-view pose is ill-determined." % (i, c2[i, 1], c2[i, 0]))
            out.append(m[masks[i]])
    return out, [(int(kind[i]), int(counts[i]), int(c2[i, 0]), int(c2[i, 1]), F[i], Hm[i]) for i in range(len(blocks))]


POSE_MIN_INLIERS = 15        # find_transform's gates (NViewReconstuct.cpp:1041, 1056): more inliers than this,
POSE_MIN_FRONT = 0.7         # and at least this share of them in front of both cameras


def _normalised_blocks(K, key_points_for_all, matches_for_all):
    """per consecutive pair the rows (x1, y1, x2, y2) of its matches normalised by K"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    blocks = []
    for i, m in enumerate(matches_for_all):
        a, b = key_points_for_all[i], key_points_for_all[i + 1]
        q, t = m["queryIdx"], m["trainIdx"]
        blocks.append(np.stack([(a["x"][q].astype(np.float64) - cx) / fx, (a["y"][q].astype(np.float64) - cy) / fy,
                                (b["x"][t].astype(np.float64) - cx) / fx, (b["y"][t].astype(np.float64) - cy) / fy], 1).reshape(-1, 4))
    return blocks, 0.5 * (fx + fy)


def relative_pose_for_all(K, key_points_for_all, matches_for_all, px=1.0, px_h=2.0, hypotheses=1024, rounds=3, seed=0, min_inliers=15, hf_ratio=0.8,
                          pose_rounds=3, pose_iters=10, max_depth=50.0, min_angle_deg=2.0, ctx=None):
    """find_transform (NViewReconstuct.cpp:1022-1060) for every consecutive pair of the chain on the device: two_view_geometry (F and
    homography RANSAC, the selection) and then relative_pose on the pairs of kind 1, with F's inlier mask and F.  Returns per pair a dict:
    ok, R (3 x 3) and t (unit 3; NaN without a pose), kind (0, 1, 2 of sfmhip_two_view_geometry), counts (dict: n_used, n_inl, n_front,
    n_angle, cand, n4), sv (s0, s1, s2 of F) and kept (bool per match: the final inliers in front of both cameras, bit 1 of mask_out).
    ok applies find_transform's own gates, more than 15 inliers and n_front / n_inl >= 0.7, and requires kind 1; a pair of kind 0 or 2 is
    reported without a pose (a pose from the homography is not provided)."""
    ctx = ctx or default_context()
    blocks, f = _normalised_blocks(K, key_points_for_all, matches_for_all)
    if not blocks:
        return []
    kind, masks, _, _, F, _, _ = ctx.two_view_geometry(blocks, px / f, px_h / f, hypotheses, rounds, seed, min_inliers, hf_ratio)
    general = [q for q in range(len(blocks)) if kind[q] == 1]
    out = [dict(ok=False, R=np.full((3, 3), np.nan), t=np.full(3, np.nan), kind=int(kind[q]), counts=dict(n_used=0, n_inl=0, n_front=0, n_angle=0, cand=-1, n4=[0] * 4),
                sv=np.full(3, np.nan), kept=np.zeros(len(blocks[q]), bool)) for q in range(len(blocks))]
    if general:
        pose, info, quality, mo = ctx.relative_pose([blocks[q] for q in general], [masks[q] for q in general], F[general], px / f, pose_rounds, pose_iters,
                                                    max_depth, min_angle_deg)
        for j, q in enumerate(general):
            o, i = out[q], info[j]
            o["counts"] = dict(n_used=int(i[6]), n_inl=int(i[7]), n_front=int(i[8]), n_angle=int(i[9]), cand=int(i[1]), n4=[int(x) for x in i[2:6]])
            o["sv"] = quality[j, :3].copy()
            if i[0] == 1:
                o["R"] = pose[j, :9].reshape(3, 3).copy(); o["t"] = pose[j, 9:].copy()
                o["kept"] = (mo[j] & 2) != 0
                o["ok"] = bool(i[7] > POSE_MIN_INLIERS and i[8] >= POSE_MIN_FRONT * i[7])
    return out


SV_RATIO_MAX = 2.0           # a P whose left block has S0 / S2 above this is not a pose (coplanar points); the measured ranges: DESIGN.md 4c


def pose_from_projection(P):
    """(ok, R 3 x 3, t 3, sv_ratio) of a winner of register_views on normalised observations (sfmhip_pose_from_projection, host code);
    ok False with NaN outputs for a non-finite P, a degenerate block or a reflection"""
    P = np.ascontiguousarray(P, np.float64).reshape(12)
    R = np.full((3, 3), np.nan); t = np.full(3, np.nan); sv = C.c_double(np.nan)
    rc = _lib.load().sfmhip_pose_from_projection(P.ctypes.data, R.ctypes.data, t.ctypes.data, C.byref(sv))
    return rc == _lib.OK, R, t, sv.value


def _rvec_of(R):
    """the angle-axis vector of a rotation matrix away from a half turn (the logarithm of cv::Rodrigues)"""
    th = np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return 0.5 * w if th < 1e-12 else th * w / (2.0 * np.sin(th))


def _rotmat_of(aa):
    th = np.linalg.norm(aa)
    if th < 1e-15:
        return np.eye(3)
    w = aa / th
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def register_views_for_all(K, obj_pts_list, img_pts_list, px=2.0, hypotheses=1024, rounds=3, seed=0, min_inliers=6, sv_ratio_max=SV_RATIO_MAX,
                           ctx=None):
    """cv::solvePnPRansac (NViewReconstuct.cpp:1415) for many views in one call: obj_pts_list[q] (m_q, 3) structure points and
    img_pts_list[q] (m_q, 2) their pixel observations in view q.  The observations are normalised by K, register_views runs at px pixels,
    the pose comes out of the winning P (pose_from_projection) and is polished on the inliers by the motion-only bundle
    adjustment: one camera, every point constant, intrinsics fixed.  Returns per view (ok, R 3 x 3, t 3, mask bool m_q, count,
    sv_ratio); ok is False, with the mask and count still reported, where there is no model, P is no rotation, or sv_ratio exceeds
    sv_ratio_max (coplanar points: the DLT's P is not a pose there)."""
    ctx = ctx or default_context()
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    blocks = []
    for X, uv in zip(obj_pts_list, img_pts_list):
        X = np.asarray(X, np.float64).reshape(-1, 3); uv = np.asarray(uv, np.float64).reshape(-1, 2)
        blocks.append(np.column_stack([X, (uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy]))
    if not blocks:
        return []
    masks, counts, P, _ = ctx.register_views(blocks, px / (0.5 * (fx + fy)), hypotheses, rounds, seed, min_inliers)
    out = []
    for q, b in enumerate(blocks):
        ok, R, t, sv = (False, np.full((3, 3), np.nan), np.full(3, np.nan), np.nan) if counts[q] == 0 else pose_from_projection(P[q])
        ok = bool(ok and sv <= sv_ratio_max)
        if ok:
            m = masks[q]
            n = int(m.sum())
            uv = np.asarray(img_pts_list[q], np.float64).reshape(-1, 2)[m]
            o = ctx.ba_options(fix_first_camera=0, fix_intrinsics=1)
            _, ext, _, s = ctx.ba_solve([fx, fy, cx, cy], np.concatenate([_rvec_of(R), t])[None], b[m, :3], np.zeros(n, np.int32),
                                        np.arange(n, dtype=np.int32), uv, o, cam_const=np.zeros(1, bool), pt_const=np.ones(n, bool))
            if s["termination"] != 2 and np.isfinite(ext).all():
                R, t = _rotmat_of(ext[0, :3]), ext[0, 3:].copy()
        out.append((ok, R, t, masks[q], int(counts[q]), float(sv)))
    return out


def get_matched_points(p1, p2, matches):
    """NViewReconstuct.cpp:989-1003 on KEYPOINT arrays."""
    return (np.stack([p1["x"][matches["queryIdx"]], p1["y"][matches["queryIdx"]]], 1).astype(np.float32),
            np.stack([p2["x"][matches["trainIdx"]], p2["y"][matches["trainIdx"]]], 1).astype(np.float32))


def projection_matrix(K, R, T):
    """NViewReconstuct.cpp:1129-1143: float32(K) @ [float32(R) | float32(T)] (float32 cv::Mat product:
    each dot product accumulated in double and rounded once [3P])."""
    fK = np.asarray(K, np.float64).reshape(3, 3).astype(np.float32)
    RT = np.concatenate([np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(3, 1)], 1).astype(np.float32)
    return (fK.astype(np.float64) @ RT.astype(np.float64)).astype(np.float32)


def reconstruct(K, R1, T1, R2, T2, p1, p2, ctx=None):
    """NViewReconstuct.cpp:1117-1159.  Returns (ret, structure): ret = -1 and an "[Err]" line on empty input."""
    p1 = np.asarray(p1, np.float32).reshape(-1, 2); p2 = np.asarray(p2, np.float32).reshape(-1, 2)
    if p1.shape[0] == 0 or p2.shape[0] == 0:
        print("[Err]: empty 2d points.")
        return -1, np.zeros((0, 3))
    ctx = ctx or default_context()
    _, xyz = ctx.triangulate2(projection_matrix(K, R1, T1), projection_matrix(K, R2, T2), p1, p2)
    return 0, xyz


def bundle_adjustment(intrinsic, extrinsics, correspond_struct_idx, key_points_for_all, structure, ctx=None, opts=None,
                      const_cameras=None, const_points=None):
    """NViewReconstuct.cpp:1162-1244.  intrinsic (4,), extrinsics (n_cam,6), structure (n_pt,3) are updated IN PLACE
    (numpy float64 arrays); correspond_struct_idx[img][kp] = point id or -1; key_points_for_all[img] = KEYPOINT array
    or (n,2) float array.  const_cameras / const_points: index lists of blocks held constant (on top of camera 0 while
    opts.fix_first_camera is set; sfmhip_ba_solve_ex).  Returns the summary dict and prints the reference's statistics block."""
    ctx = ctx or default_context()
    oc, op, uv = [], [], []
    for img, ids in enumerate(correspond_struct_idx):
        ids = np.asarray(ids)
        kp = key_points_for_all[img]
        xy = np.stack([kp["x"], kp["y"]], 1) if getattr(kp, "dtype", None) is not None and kp.dtype.names else np.asarray(kp)
        sel = np.nonzero(ids >= 0)[0]
        oc.append(np.full(sel.shape[0], img, np.int32)); op.append(ids[sel].astype(np.int32))
        uv.append(xy[sel].astype(np.float32).astype(np.float64))      # Point2d observed = key_points[pt_id].pt (1199)
    oc = np.concatenate(oc); op = np.concatenate(op); uv = np.concatenate(uv)
    n_cam, n_pt = len(extrinsics), len(structure)
    K4, ext, pts, s = ctx.ba_solve(intrinsic, extrinsics, structure, oc, op, uv, opts,
                                   cam_const=_index_mask(const_cameras, n_cam), pt_const=_index_mask(const_points, n_pt))
    np.copyto(intrinsic, K4.reshape(np.shape(intrinsic))); np.copyto(extrinsics, ext.reshape(np.shape(extrinsics)))
    np.copyto(structure, pts.reshape(np.shape(structure)))
    if s["termination"] == 2:
        print("Bundle Adjustment failed.")
    else:
        print("\nBundle Adjustment statistics (approximated RMSE):\n #views: %d\n #residuals: %d\n"
              " Initial RMSE(pixel): %g\n Final   RMSE(pixel): %g\n Time (s): %g\n"
              % (len(extrinsics), s["num_residuals"], np.sqrt(s["initial_cost"] / max(1, s["num_residuals"])),
                 np.sqrt(s["final_cost"] / max(1, s["num_residuals"])), s["total_time_s"]))
    return s


def refine_structure(intrinsic, extrinsics, obs_cam, obs_pt, obs_uv, structure, max_px=4.0, ctx=None, opts=None):
    """Extension (not reference behaviour, which never filters or re-triangulates: NViewReconstuct.cpp:1428-1453):
    drop observations whose reprojection error exceeds max_px, re-triangulate every track from all its remaining observations
    (sfmhip_triangulate_tracks), drop tracks left with fewer than two views, bundle-adjust again.
    Returns (K4, ext, pts (kept), kept point ids, kept observation mask, summary)."""
    ctx = ctx or default_context()
    K4 = np.array(intrinsic, np.float64).reshape(4); ext = np.array(extrinsics, np.float64).reshape(-1, 6)
    pts = np.array(structure, np.float64).reshape(-1, 3)
    oc = np.ascontiguousarray(obs_cam, np.int32); op = np.ascontiguousarray(obs_pt, np.int32); uv = np.ascontiguousarray(obs_uv, np.float64).reshape(-1, 2)
    err = ctx.reprojection_errors(K4, ext, pts, oc, op, uv)
    keep = err <= max_px
    new_pts, nv = ctx.triangulate_tracks(K4, ext, oc[keep], op[keep], uv[keep], len(pts))
    ok = (nv >= 2) & np.isfinite(new_pts).all(1)
    ids = np.nonzero(ok)[0]
    remap = np.full(len(pts), -1, np.int64); remap[ids] = np.arange(len(ids))
    keep &= ok[op]
    K2, ext2, pts2, s = ctx.ba_solve(K4, ext, new_pts[ids], oc[keep], remap[op[keep]].astype(np.int32), uv[keep], opts)
    return K2, ext2, pts2, ids, keep, s


# ---------------------------------------------------------------------------------------------------- dense depth
def _dense_images(images):
    """(arrays, addresses, rows, cols, channels, ld) of uint8 images of one size for the dense entries: an image whose pixels are
    contiguous inside its rows is passed where it lies with its row stride (a view of a padded buffer), anything else as a dense copy"""
    arrs = [np.asarray(im) for im in images]
    shape = arrs[0].shape
    if len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 3) or any(a.shape != shape or a.dtype != np.uint8 for a in arrs):
        raise ValueError("images are uint8 arrays of one size, rows x cols or rows x cols x 3")
    rows, cols = shape[:2]
    ch = 1 if len(shape) == 2 else 3

    def in_place(a):
        return a.strides[-1] == 1 and (ch == 1 or a.strides[1] == 3) and a.strides[0] >= cols * ch
    if not (all(in_place(a) for a in arrs) and len({a.strides[0] for a in arrs}) == 1):
        arrs = [np.ascontiguousarray(a) for a in arrs]
    return arrs, [a.ctypes.data for a in arrs], rows, cols, ch, arrs[0].strides[0]


def sweep_geometry(K4, ext_ref, ext_src):
    """sfmhip_sweep_geometry (host only, no context): (A, b, Rrel, trel, Rinv, c)"""
    K4 = np.ascontiguousarray(K4, np.float64).reshape(4); ext_ref = np.ascontiguousarray(ext_ref, np.float64).reshape(6)
    ext_src = np.ascontiguousarray(ext_src, np.float64).reshape(-1, 6)
    n = ext_src.shape[0]
    A = np.zeros((n, 9), np.float32); b = np.zeros((n, 3), np.float32); Rrel = np.zeros((n, 9)); trel = np.zeros((n, 3)); Rinv = np.zeros(9); c = np.zeros(3)
    rc = _lib.load().sfmhip_sweep_geometry(K4.ctypes.data, ext_ref.ctypes.data, ext_src.ctypes.data, n, A.ctypes.data, b.ctypes.data, Rrel.ctypes.data,
                                           trel.ctypes.data, Rinv.ctypes.data, c.ctypes.data)
    if rc != 0:
        raise SfmHipError(f"sfmhip_sweep_geometry: error {rc}")
    return A, b, Rrel, trel, Rinv, c


def dense_sources(ext, n_src):
    """for every view the n_src other views with the nearest camera centres, nearest first (equal distances: the lower index)"""
    ext = np.ascontiguousarray(ext, np.float64).reshape(-1, 6)
    cen = np.array([sweep_geometry((1.0, 1.0, 0.0, 0.0), e, np.zeros((0, 6)))[5] for e in ext])
    out = []
    for i in range(len(ext)):
        d = np.sqrt(((cen - cen[i]) ** 2).sum(1)); d[i] = np.inf
        out.append([int(j) for j in np.argsort(d, kind="stable")[:n_src]])
    return out


def dense_depth_range(sparse_pts, ext6):
    """[wmin, wmax] of a view from the depths z > 0 of the sparse points in it: the inverses of their 98th and 2nd percentile, the
    interval then widened by a quarter of its length at both ends (the lower end no lower than half the 98th percentile's inverse)"""
    _, _, _, _, Rinv, c = sweep_geometry((1.0, 1.0, 0.0, 0.0), ext6, np.zeros((0, 6)))
    P = np.ascontiguousarray(sparse_pts, np.float64).reshape(-1, 3)
    z = ((P[:, 0] - c[0]) * Rinv[2] + (P[:, 1] - c[1]) * Rinv[5]) + (P[:, 2] - c[2]) * Rinv[8]
    z = z[np.isfinite(z) & (z > 0)]
    if z.size < 2:
        raise ValueError("fewer than two sparse points in front of a view: give wmin and wmax")
    zlo, zhi = np.percentile(z, [2.0, 98.0])
    wlo, whi = 1.0 / zhi, 1.0 / zlo
    span = whi - wlo
    if not span > 0:
        span = 0.5 * wlo
    return max(wlo - 0.25 * span, 0.5 * wlo), whi + 0.25 * span


SelectedViews = collections.namedtuple("SelectedViews", "shared score sources n_scored wrange n_depth")


def select_cos2(min_angle_deg):
    """cos^2 of the smallest triangulation angle that counts, the form sfmhip_select_views takes (0 <= angle <= 90 degrees)"""
    a = float(min_angle_deg)
    if not 0.0 <= a <= 90.0:
        raise ValueError("min_angle_deg lies in [0, 90]")
    c = math.cos(a * (math.pi / 180.0))
    return c * c


def select_views(ext, pts, obs_cam, obs_pt, n_src=2, min_angle_deg=1.0, ctx=None):
    """Context.select_views on the given or a new context: SelectedViews(shared, score, sources, n_scored, wrange, n_depth)"""
    own = ctx is None
    ctx = ctx or Context(0)
    try:
        return ctx.select_views(ext, pts, obs_cam, obs_pt, n_src, min_angle_deg)
    finally:
        if own:
            ctx.close()


Tracks = collections.namedtuple("Tracks", "correspond_struct_idx obs_cam obs_pt obs_kp obs_uv track_len stats matches_for_all")


def _tracks_flags(min_len, conflicts):
    """the flags of sfmhip_build_tracks for conflicts = "drop" (OpenMVG's rule) or "keep-first"; min_len is at least 2"""
    if conflicts not in _lib.TRACKS_CONFLICTS:
        raise ValueError('conflicts is "drop" or "keep-first"')
    if int(min_len) != min_len or int(min_len) < 2:
        raise ValueError("min_len is an integer, at least 2")
    return _lib.TRACKS_CONFLICTS[conflicts]


def _tracks_inputs(key_points_for_all, pairs, matches_for_all):
    """(n_kp, pairs (n_pairs, 2), matches (n_pairs, max_per_pair) padded with -1, counts) of a list of DMATCH arrays; pairs=None: the chain"""
    n_img = len(key_points_for_all)
    if n_img < 1:
        raise ValueError("at least one image")
    n_kp = np.array([len(k) for k in key_points_for_all], np.int32)
    if pairs is None:
        pairs = np.stack([np.arange(n_img - 1), np.arange(1, n_img)], axis=1)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    if len(matches_for_all) != len(pairs):
        raise ValueError("one match list per pair (pairs=None: the chain (i, i + 1))")
    if len(pairs) and (pairs.min() < 0 or pairs.max() >= n_img or (pairs[:, 0] == pairs[:, 1]).any()):
        raise ValueError("a pair names two different images of key_points_for_all")
    lists = [np.ascontiguousarray(m, DMATCH).ravel() for m in matches_for_all]
    S = max([len(m) for m in lists], default=0)
    matches = np.zeros((len(pairs), S), DMATCH)
    matches["queryIdx"] = -1; matches["trainIdx"] = -1; matches["imgIdx"] = -1
    for q, m in enumerate(lists):
        matches[q, :len(m)] = m
    return n_kp, pairs, matches, np.array([len(m) for m in lists], np.int32)


def tracks_for_all(key_points_for_all, pairs, matches_for_all, min_len=2, conflicts="drop", ctx=None):
    """Tracks from the match lists of ANY pair list (sfmhip_build_tracks, where the definition is): the connected components of the match
    graph, conflicting components dropped (conflicts="drop", OpenMVG's rule) or cut down to one key point per image ("keep-first"), tracks
    shorter than min_len left out.  matches_for_all[q] is the DMATCH array of pairs[q] = (query image, train image) as
    match_features_for_all returns them; pairs=None is the chain (i, i + 1).  key_points_for_all[img]: KEYPOINT array or (n, 2) array.
    Returns Tracks(correspond_struct_idx, obs_cam, obs_pt, obs_kp, obs_uv, track_len, stats, matches_for_all): one int32 array per image
    with the track of every key point or -1 (what bundle_adjustment takes), the observation lists in (track, image) order, the length of
    every track, the eight counters of the C call, and the match lists reduced to the elements between two observations of a track."""
    flags_ok = _tracks_flags(min_len, conflicts); del flags_ok
    n_kp, pairs, matches, counts = _tracks_inputs(key_points_for_all, pairs, matches_for_all)
    structured = all(getattr(k, "dtype", None) is not None and k.dtype.names for k in key_points_for_all)
    ctx = ctx or default_context()
    track_of, oc, op, ok, uv, tl, stats, mo, co = ctx.build_tracks(n_kp, pairs, matches, counts, kp=list(key_points_for_all) if structured else None,
                                                                  min_len=min_len, conflicts=conflicts)
    if uv is None:                                    # plain coordinate arrays: the same gather on the host, nothing narrowed to float
        uv = np.zeros((len(oc), 2))
        for img in np.unique(oc):
            sel = oc == img
            uv[sel] = np.asarray(key_points_for_all[img], np.float64).reshape(-1, 2)[ok[sel]]
    off = np.concatenate([[0], np.cumsum(n_kp.astype(np.int64))])
    idx = [track_of[off[i]:off[i + 1]].copy() for i in range(len(n_kp))]
    return Tracks(idx, oc, op, ok, uv, tl, stats, [mo[q, :co[q]].copy() for q in range(len(pairs))])


def structure_from_tracks(K, extrinsics, key_points_for_all, pairs, matches_for_all, min_len=2, conflicts="drop", ctx=None):
    """tracks_for_all, then the N-view DLT of every track under the given poses (Context.triangulate_tracks).  K: 3 x 3 or (fx, fy, cx,
    cy); extrinsics (n_img, 6) angle-axis and t.  Returns (structure (n_tracks, 3), correspond_struct_idx, tracks), ready for
    bundle_adjustment"""
    K = np.asarray(K, np.float64)
    K4 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]) if K.shape == (3, 3) else K.reshape(4)
    ext = np.ascontiguousarray(extrinsics, np.float64).reshape(-1, 6)
    if len(ext) != len(key_points_for_all):
        raise ValueError("one pose per image")
    ctx = ctx or default_context()
    tr = tracks_for_all(key_points_for_all, pairs, matches_for_all, min_len, conflicts, ctx)
    structure, _ = ctx.triangulate_tracks(K4, ext, tr.obs_cam, tr.obs_pt, tr.obs_uv, len(tr.track_len))
    return structure, tr.correspond_struct_idx, tr


def _dense_depth_maps(ctx, images, K4, ext, sparse_pts, n_src, planes, radius, wmin, wmax, min_sources, min_score, min_consistent, sgm, observations=None,
                      min_angle_deg=1.0):
    """what dense_cloud_for_all and dense_mesh_for_all share: the images on the device, every view's sources and geometry arrays, and its
    depth map (plane sweep, or its semi-global form), all enqueued on the context's stream.  Returns (device, d_img, rows, cols, channels,
    sources, geometry, d_depth, min_consistent, scratch); the caller holds on to `scratch`, the sweeps' other outputs, until it has
    synchronised the context: the sweeps may still be writing them.  observations = (obs_cam, obs_pt) into sparse_pts: the sources and the
    ranges come from Context.select_views instead of the camera centres and the whole cloud."""
    import torch
    ext = np.ascontiguousarray(ext, np.float64).reshape(-1, 6)
    n_img = len(images)
    if n_img != len(ext) or n_img < 2:
        raise ValueError("one pose per image, at least two images")
    n_src = min(int(n_src), n_img - 1)
    if min_consistent is None:
        min_consistent = min(2, n_src)
    dev = torch.device("cuda", ctx.device)
    d_img = [im.to(dev).contiguous() if hasattr(im, "data_ptr") else torch.from_numpy(np.ascontiguousarray(im)).to(dev) for im in images]
    rows, cols = d_img[0].shape[:2]
    ch = 1 if d_img[0].dim() == 2 else 3
    if any(t.shape != d_img[0].shape or t.dtype != torch.uint8 for t in d_img) or (ch == 3 and d_img[0].shape[2] != 3):
        raise ValueError("images are uint8 arrays of one size, rows x cols or rows x cols x 3")
    torch.cuda.synchronize(dev)                      # the uploads ran on torch's stream, the stages run on the context's
    sel = None
    if observations is not None:
        # sources and ranges from the sparse model (sfmhip_select_views); the call drains the stream before the sweeps are enqueued
        if sparse_pts is None:
            raise ValueError("observations index sparse_pts: give both")
        sel = ctx.select_views(ext, sparse_pts, observations[0], observations[1], n_src, min_angle_deg)
        sources = [[int(j) for j in row] for row in sel.sources]
        if (wmin is None or wmax is None) and (sel.n_depth < 2).any():
            raise ValueError("fewer than two sparse points in front of a view: give wmin and wmax")
    else:
        sources = dense_sources(ext, n_src)
    geo = [sweep_geometry(K4, ext[i], ext[sources[i]]) for i in range(n_img)]
    npx = rows * cols
    d_depth = [torch.empty(npx, dtype=torch.float32, device=dev) for _ in range(n_img)]
    d_plane = torch.empty(npx, dtype=torch.int32, device=dev); d_score = torch.empty(npx, dtype=torch.float32, device=dev)
    d_cost = torch.empty(npx if sgm is not None else 0, dtype=torch.int16, device=dev)       # the winners' 16-bit costs
    for i in range(n_img):
        if wmin is not None and wmax is not None:
            lo, hi = wmin, wmax
        elif sel is None:
            lo, hi = dense_depth_range(sparse_pts, ext[i])
        else:
            lo, hi = (float(x) for x in sel.wrange[i])
        if sgm is not None:
            cost_scale, P1, P2, paths, max_cost = sgm
            ctx.plane_sweep_sgm_dev(d_img[i], [d_img[j] for j in sources[i]], rows, cols, ch, cols * ch, geo[i][0], geo[i][1], planes, lo, hi, radius,
                                    min_sources, cost_scale, P1, P2, paths, max_cost, d_plane, d_cost, d_depth[i])
            continue
        ctx.plane_sweep_dev(d_img[i], [d_img[j] for j in sources[i]], rows, cols, ch, cols * ch, geo[i][0], geo[i][1], planes, lo, hi, radius, min_sources,
                            min_score, d_plane, d_score, d_depth[i])
    return dev, d_img, rows, cols, ch, sources, geo, d_depth, min_consistent, (d_plane, d_score, d_cost)


def dense_cloud_for_all(images, K4, ext, sparse_pts=None, n_src=2, planes=64, radius=2, wmin=None, wmax=None, min_sources=1, min_score=0.5, rel_tol=0.01,
                        min_consistent=None, voxel=0.0, ctx=None, sgm=None, observations=None, min_angle_deg=1.0):
    """The dense step after the bundle adjustment: every view is swept against the n_src views with the nearest camera centres
    (sfmhip_plane_sweep_dev), its depth map is checked against theirs (sfmhip_depth_consistency_dev), the kept pixels become coloured
    world points (sfmhip_depth_to_points_dev), and the views' points are concatenated in view order.  images: uint8 arrays (or torch
    CUDA tensors) of one size, gray or BGR; K4 and ext: the bundle adjustment's intrinsics and (angle-axis, t) rows.  The inverse-depth
    range of a view comes from sparse_pts (dense_depth_range) unless wmin and wmax are given.  min_consistent: min(2, n_src) unless
    given.  voxel > 0: the cloud is replaced by one centroid per voxel (voxel_downsample; a voxel's colour is the rounded mean of its
    points' per channel).  sgm = (cost_scale, P1, P2, paths, max_cost): the sweep's costs are aggregated along 4 or 8 directions before
    the winner is taken (sfmhip_plane_sweep_sgm_dev; at most 256 planes, min_score is not used); None: the winner per pixel.  The
    images, depth maps and masks stay on the device between the stages.  observations = (obs_cam, obs_pt), the bundle adjustment's lists
    into sparse_pts: every view is swept against the n_src views it shares the most sparse points with under at least min_angle_deg of
    triangulation angle, over the depths of the points it sees (sfmhip_select_views); wmin and wmax, where given, still set the range.
    Returns (xyz n x 3 float64, bgr n x 3 uint8)."""
    import torch
    own = ctx is None
    ctx = ctx or Context(0)
    try:
        dev, d_img, rows, cols, ch, sources, geo, d_depth, min_consistent, scratch = _dense_depth_maps(ctx, images, K4, ext, sparse_pts, n_src, planes, radius, wmin, wmax,
                                                                                                         min_sources, min_score, min_consistent, sgm, observations,
                                                                                                         min_angle_deg)
        n_img, npx = len(d_img), rows * cols
        d_keep = torch.empty(npx, dtype=torch.uint8, device=dev)
        d_xyz = torch.empty((npx, 3), dtype=torch.float64, device=dev); d_bgr = torch.empty((npx, 3), dtype=torch.uint8, device=dev)
        d_n = torch.empty(1, dtype=torch.int32, device=dev)
        xyz, bgr = [], []
        for i in range(n_img):
            _, _, Rrel, trel, Rinv, c = geo[i]
            ctx.depth_consistency_dev(d_depth[i], [d_depth[j] for j in sources[i]], rows, cols, K4, Rrel, trel, rel_tol, min_consistent, None, d_keep)
            ctx.depth_to_points_dev(d_depth[i], d_keep, d_img[i], rows, cols, ch, cols * ch, K4, Rinv, c, d_xyz, d_bgr, npx, d_n)
            ctx.synchronize()
            m = int(d_n.item())
            xyz.append(d_xyz[:m].cpu().numpy()); bgr.append(d_bgr[:m].cpu().numpy())
        xyz = np.concatenate(xyz); bgr = np.concatenate(bgr)
        if voxel and voxel > 0 and len(xyz):
            cen, counts, voxel_of, _ = ctx.voxel_downsample(xyz, voxel)
            total = np.zeros((len(cen), 3), np.int64)
            ok = voxel_of >= 0
            np.add.at(total, voxel_of[ok], bgr[ok].astype(np.int64))
            cnt = counts.astype(np.int64)[:, None]
            xyz, bgr = cen, ((2 * total + cnt) // (2 * cnt)).astype(np.uint8)
        return xyz, bgr
    finally:
        if own:
            ctx.close()


# ---------------------------------------------------------------------------------------------------- dense mesh
def _tsdf_volume_ok(dims, dsum, wsum, csum):
    nvox = int(dims[0]) * int(dims[1]) * int(dims[2])
    for a, dt, shape in ((dsum, np.int32, (nvox,)), (wsum, np.int32, (nvox,)), (csum, np.uint32, (nvox, 3))):
        if a is not None and not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous and a.size == int(np.prod(shape))):
            raise ValueError("the volume is contiguous arrays: dsum, wsum int32 of nx*ny*nz entries, csum uint32 of three per voxel")


def _tsdf_host_args(dims, origin, K4, R, t, n):
    return (np.ascontiguousarray(dims, np.int32).reshape(3), np.ascontiguousarray(origin, np.float64).reshape(3), np.ascontiguousarray(K4, np.float64).reshape(4),
            np.ascontiguousarray(R, np.float64).reshape(n, 9), np.ascontiguousarray(t, np.float64).reshape(n, 3))


def tsdf_bounds(sparse_pts, voxels=128, margin=0.1):
    """(dims, origin, voxel) of a volume around the sparse cloud: per axis the 2nd and 98th percentile of the finite points, the interval
    widened by `margin` of its length at both ends; the voxel is the longest side over `voxels`, and the other axes take as many voxels as
    cover their side (at least 2), centred on it"""
    P = np.ascontiguousarray(sparse_pts, np.float64).reshape(-1, 3)
    P = P[np.isfinite(P).all(1)]
    if len(P) < 2:
        raise ValueError("fewer than two finite sparse points: give the volume")
    lo, hi = np.percentile(P, 2.0, axis=0), np.percentile(P, 98.0, axis=0)
    span = hi - lo
    lo, hi = lo - float(margin) * span, hi + float(margin) * span
    side = hi - lo
    if not side.max() > 0:
        raise ValueError("the sparse points do not span a volume")
    voxel = float(side.max()) / int(voxels)
    dims = np.maximum(np.ceil(side / voxel - 1e-9).astype(np.int64), 2)
    origin = 0.5 * (lo + hi) - 0.5 * dims * voxel
    return tuple(int(d) for d in dims), tuple(float(o) for o in origin), voxel


def dense_mesh_for_all(images, K4, ext, sparse_pts=None, n_src=2, planes=64, radius=2, wmin=None, wmax=None, min_sources=1, min_score=0.5, rel_tol=0.01,
                       min_consistent=None, ctx=None, voxels=128, trunc_voxels=4, min_weight=2, sgm=None, volume=None, min_component=None, keep_largest=False,
                       simplify_voxels=None, smooth=None, normals=False, observations=None, min_angle_deg=1.0):
    """The dense surface after the bundle adjustment: the depth maps and keep masks of dense_cloud_for_all's chain (same arguments, same
    meaning) stay on the device, all views are fused into one truncated signed distance volume 8 per call (sfmhip_tsdf_integrate_dev) and
    the volume is meshed by marching tetrahedra (sfmhip_tsdf_mesh_dev, once for the counts and once into arrays of that size).  The
    volume is volume = (dims, origin, voxel) or tsdf_bounds(sparse_pts, voxels); the truncation distance trunc_voxels voxels; a voxel
    counts with min_weight views.  Returns (xyz n x 3 float64, bgr n x 3 uint8, tri m x 3 int32).
    The clean-up of the resident mesh, every step off by default and run in this order: min_component / keep_largest (the components with
    at least that many triangles / only the largest: sfmhip_mesh_filter_components_dev), simplify_voxels (vertex clustering on cells of that
    many voxels: sfmhip_mesh_simplify_dev), smooth = (iterations, lambda, mu) (sfmhip_mesh_smooth_dev), normals (a fourth array, n x 3
    float64: sfmhip_mesh_vertex_normals_dev)."""
    import torch
    own = ctx is None
    ctx = ctx or Context(0)
    try:
        dev, d_img, rows, cols, ch, sources, geo, d_depth, min_consistent, scratch = _dense_depth_maps(ctx, images, K4, ext, sparse_pts, n_src, planes, radius, wmin, wmax,
                                                                                                         min_sources, min_score, min_consistent, sgm, observations,
                                                                                                         min_angle_deg)
        n_img, npx = len(d_img), rows * cols
        dims, origin, voxel = volume if volume is not None else tsdf_bounds(sparse_pts, voxels)
        nvox = int(dims[0]) * int(dims[1]) * int(dims[2])
        d_keep = [torch.empty(npx, dtype=torch.uint8, device=dev) for _ in range(n_img)]
        for i in range(n_img):
            ctx.depth_consistency_dev(d_depth[i], [d_depth[j] for j in sources[i]], rows, cols, K4, geo[i][2], geo[i][3], rel_tol, min_consistent, None, d_keep[i])
        ctx.synchronize()                                # the volume is zeroed on torch's stream
        d_dsum = torch.zeros(nvox, dtype=torch.int32, device=dev); d_wsum = torch.zeros(nvox, dtype=torch.int32, device=dev)
        d_csum = torch.zeros((nvox, 3), dtype=torch.int32, device=dev)
        d_n = torch.zeros(2, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        # world to camera of every view: Rinv = R^T and c = -R^T t from the geometry call
        R = np.array([np.asarray(g[4]).reshape(3, 3).T.ravel() for g in geo])
        t = np.ascontiguousarray(ext, np.float64).reshape(-1, 6)[:, 3:]
        for i0 in range(0, n_img, 8):
            sl = slice(i0, min(i0 + 8, n_img))
            ctx.tsdf_integrate_dev(dims, origin, voxel, trunc_voxels * voxel, d_depth[sl], d_keep[sl], d_img[sl], rows, cols, ch, cols * ch, K4, R[sl], t[sl],
                                   d_dsum, d_wsum, d_csum)
        ctx.tsdf_mesh_dev(dims, origin, voxel, d_dsum, d_wsum, d_csum, min_weight, None, None, 0, None, 0, d_n[0:1], d_n[1:2])
        ctx.synchronize()
        nv, nt = (int(x) for x in d_n.cpu().numpy())
        d_xyz = torch.empty((max(nv, 1), 3), dtype=torch.float64, device=dev); d_bgr = torch.empty((max(nv, 1), 3), dtype=torch.uint8, device=dev)
        d_tri = torch.empty((max(nt, 1), 3), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        ctx.tsdf_mesh_dev(dims, origin, voxel, d_dsum, d_wsum, d_csum, min_weight, d_xyz, d_bgr, nv, d_tri, nt, d_n[0:1], d_n[1:2])
        ctx.synchronize()

        def rebuilt(call, *params):
            """a call that writes a new mesh: the arrays it filled and their counts"""
            o_xyz = torch.empty((max(nv, 1), 3), dtype=torch.float64, device=dev); o_bgr = torch.empty((max(nv, 1), 3), dtype=torch.uint8, device=dev)
            o_tri = torch.empty((max(nt, 1), 3), dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            call(d_xyz, d_bgr, nv, d_tri, nt, *params, o_xyz, o_bgr, o_tri, None, d_n[0:1], d_n[1:2])
            ctx.synchronize()
            mv, mt = (int(x) for x in d_n.cpu().numpy())
            if mv < 0:
                raise SfmHipError("dense_mesh_for_all: the mesh clean-up failed (a cluster cell too small for the mesh's extent, or the union-find's retry cap)")
            return o_xyz, o_bgr, o_tri, mv, mt
        if min_component is not None or keep_largest:
            d_xyz, d_bgr, d_tri, nv, nt = rebuilt(ctx.mesh_filter_components_dev, 1 if min_component is None else int(min_component), bool(keep_largest))
        if simplify_voxels is not None:
            d_xyz, d_bgr, d_tri, nv, nt = rebuilt(ctx.mesh_simplify_dev, float(simplify_voxels) * voxel)
        if smooth is not None:
            iterations, lam, mu = smooth
            o_xyz = torch.empty((max(nv, 1), 3), dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)
            ctx.mesh_smooth_dev(d_xyz, nv, d_tri, nt, iterations, lam, mu, o_xyz)
            ctx.synchronize()
            d_xyz = o_xyz
        out = (d_xyz[:nv].cpu().numpy(), d_bgr[:nv].cpu().numpy(), d_tri[:nt].cpu().numpy())
        if normals:
            d_nrm = torch.empty((max(nv, 1), 3), dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)
            ctx.mesh_vertex_normals_dev(d_xyz, nv, d_tri, nt, d_nrm)
            ctx.synchronize()
            out += (d_nrm[:nv].cpu().numpy(),)
        return out
    finally:
        if own:
            ctx.close()
