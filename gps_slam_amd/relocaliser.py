"""Keyframe relocaliser (InfiniTAM's FernRelocLib) on the device: a thin wrapper over the gps_reloc_* C ABI.

    FernRelocaliser.process_frame   Relocaliser::ProcessFrame (Relocaliser.h:48-84): subsample x 4, blur, fern code, k nearest stored
                                    codes, keyframe harvesting -- four stream-ordered launches on the current stream, nothing read back
    FernRelocaliser.read_result     the frame's result record (synchronises the stream)
    FernRelocaliser.retrieve_pose   PoseDatabase::retrievePose
    export_database / import_database   the code matrix, the poses and the scene ids as host arrays

There is no host restatement here: every step is a HIP kernel, and a missing library is an error.
"""
import ctypes as C

import numpy as np
import torch

from ._lib import RelocResult, check, lib

MAX_K = 4


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def gaussian_taps(sigma=2.5):
    """createGaussianFilter (PixelUtils.h:9-13) with filterGaussian's mask size (:158-159) -> float32[taps]; host code"""
    coeff = np.zeros(32, np.float32)
    n = C.c_int(0)
    check(lib.gps_reloc_gaussian_taps(float(sigma), 32, coeff.ctypes.data, C.addressof(n)), "gps_reloc_gaussian_taps")
    return coeff[:n.value].copy()


def default_ferns(width, height, num_ferns=500, num_decisions=4, depth_range=(0.2, 3.0), seed=0):
    """the library's default fern table for a seed -> (xy int32[n,2], thresholds float32[n]), n = num_ferns * num_decisions; host code"""
    n = int(num_ferns) * int(num_decisions)
    xy, thr = np.zeros((max(n, 0), 2), np.int32), np.zeros(max(n, 0), np.float32)
    check(lib.gps_reloc_default_ferns(int(width), int(height), int(num_ferns), int(num_decisions), float(depth_range[0]),
                                      float(depth_range[1]), int(seed), xy.ctypes.data, thr.ctypes.data), "gps_reloc_default_ferns")
    return xy, thr


class FernRelocaliser:
    """One gps_reloc_state.  depth_range: the thresholds' range (the engine passes viewFrustum_min / max); harvesting_threshold
    0.2, 500 ferns of 4 decisions: ITMBasicEngine.tpp:57-60."""

    def __init__(self, width, height, depth_range=(0.2, 3.0), harvesting_threshold=0.2, num_ferns=500, num_decisions=4,
                 capacity=4096, seed=0, device="cuda"):
        self.device = torch.device(device)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.gps_reloc_create(C.byref(self._h), int(width), int(height), int(num_ferns), int(num_decisions),
                                       float(depth_range[0]), float(depth_range[1]), float(harvesting_threshold), int(capacity),
                                       int(seed)), "gps_reloc_create")
        info = (C.c_int32 * 8)()
        check(lib.gps_reloc_info(self._h, info), "gps_reloc_info")
        (self.width, self.height, self.small_width, self.small_height, self.num_ferns, self.num_decisions, self.capacity,
         self.taps) = [int(v) for v in info]
        self._dbg = None

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            torch.cuda.synchronize(self.device)
            check(lib.gps_reloc_destroy(self._h), "gps_reloc_destroy")
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- fern table
    def set_ferns(self, xy, thresholds):
        xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        thr = np.ascontiguousarray(thresholds, np.float32).reshape(-1)
        if xy.shape[0] != thr.shape[0]:
            raise ValueError("set_ferns: %d locations against %d thresholds" % (xy.shape[0], thr.shape[0]))
        check(lib.gps_reloc_set_ferns(self._h, xy.ctypes.data, thr.ctypes.data, int(thr.shape[0]), _stream(self.device)),
              "gps_reloc_set_ferns")

    def ferns(self):
        n = self.num_ferns * self.num_decisions
        xy, thr = np.zeros((n, 2), np.int32), np.zeros(n, np.float32)
        check(lib.gps_reloc_get_ferns(self._h, xy.ctypes.data, thr.ctypes.data, n), "gps_reloc_get_ferns")
        return xy, thr

    # ---- per frame
    def enable_debug_outputs(self, on=True):
        """every later frame also leaves its blurred image and its code in self.blurred / self.code (device tensors)"""
        if on:
            self.blurred = torch.zeros((self.small_height, self.small_width), dtype=torch.float32, device=self.device)
            self.code = torch.zeros(self.num_ferns, dtype=torch.uint8, device=self.device)
            self._dbg = (self.blurred, self.code)
            check(lib.gps_reloc_set_debug_outputs(self._h, self.blurred.data_ptr(), self.code.data_ptr()), "gps_reloc_set_debug_outputs")
        else:
            torch.cuda.synchronize(self.device)
            check(lib.gps_reloc_set_debug_outputs(self._h, None, None), "gps_reloc_set_debug_outputs")
            self._dbg = None

    def process_frame(self, depth, pose_M, pose_invM, scene_id=0, k=1, harvest=True):
        """depth: float32 [H,W] device tensor in metres (<= 0: hole); pose_M / pose_invM: 16 floats each, ORUtils layout.  Enqueues
        the frame on the current stream and returns at once; read_result() fetches what it found."""
        if not (depth.is_cuda and depth.dtype == torch.float32 and depth.is_contiguous() and
                tuple(depth.shape) == (self.height, self.width)):
            raise ValueError("depth must be a contiguous float32 [%d,%d] device tensor" % (self.height, self.width))
        M = np.ascontiguousarray(pose_M, np.float32).reshape(-1)
        iM = np.ascontiguousarray(pose_invM, np.float32).reshape(-1)
        if M.size != 16 or iM.size != 16:
            raise ValueError("pose_M and pose_invM must hold 16 floats each")
        check(lib.gps_reloc_process_frame(self._h, depth.data_ptr(), M.ctypes.data, iM.ctypes.data, int(scene_id), int(k),
                                          1 if harvest else 0, _stream(self.device)), "gps_reloc_process_frame")

    def read_result(self):
        """-> dict(added_id, n_found, ids[4], distances[4], n_entries, overflow) of the last frame enqueued on the current stream"""
        r = RelocResult()
        check(lib.gps_reloc_read_result(self._h, C.byref(r), _stream(self.device)), "gps_reloc_read_result")
        return dict(added_id=int(r.added_id), n_found=int(r.n_found), ids=[int(v) for v in r.ids],
                    distances=np.array(list(r.distances), np.float32), n_entries=int(r.n_entries), overflow=int(r.overflow))

    def retrieve_pose(self, idx):
        M, iM, sc = np.zeros(16, np.float32), np.zeros(16, np.float32), C.c_int32(0)
        check(lib.gps_reloc_retrieve_pose(self._h, int(idx), M.ctypes.data, iM.ctypes.data, C.addressof(sc), _stream(self.device)),
              "gps_reloc_retrieve_pose")
        return M, iM, int(sc.value)

    # ---- the database as host arrays
    def counts(self):
        """-> (entries, harvests refused by a full database)"""
        n, over = C.c_int32(0), C.c_int32(0)
        check(lib.gps_reloc_export(self._h, 0, None, None, None, C.addressof(n), C.addressof(over), _stream(self.device)),
              "gps_reloc_export")
        return int(n.value), int(over.value)

    def export_database(self):
        n = self.counts()[0]
        codes, poses, scenes = np.zeros((n, self.num_ferns), np.uint8), np.zeros((n, 32), np.float32), np.zeros(n, np.int32)
        got = C.c_int32(0)
        check(lib.gps_reloc_export(self._h, n, codes.ctypes.data, poses.ctypes.data, scenes.ctypes.data, C.addressof(got), None,
                                   _stream(self.device)), "gps_reloc_export")
        return dict(codes=codes[:got.value], poses=poses[:got.value], scene_ids=scenes[:got.value])

    def import_database(self, codes, poses, scene_ids):
        codes = np.ascontiguousarray(codes, np.uint8).reshape(-1, self.num_ferns)
        n = codes.shape[0]
        poses = np.ascontiguousarray(poses, np.float32).reshape(n, 32)
        scenes = np.ascontiguousarray(scene_ids, np.int32).reshape(n)
        check(lib.gps_reloc_import(self._h, n, codes.ctypes.data, poses.ctypes.data, scenes.ctypes.data, _stream(self.device)),
              "gps_reloc_import")

    def guards_intact(self):
        """the bytes directly behind the code matrix, the poses and the scene ids still carry their pattern"""
        st = lib.gps_reloc_check_guards(self._h, _stream(self.device))
        if st not in (0, -3):
            check(st, "gps_reloc_check_guards")
        return st == 0
