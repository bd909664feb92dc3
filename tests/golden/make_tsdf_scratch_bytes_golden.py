"""Writes tests/golden/tsdf_scratch_bytes.json: what gps_tsdf_scratch_bytes of a given build of the library returns for a few
image and table sizes.  The committed table was recorded from the commit BEFORE the scratch layout moved into one function
(python tests/golden/make_tsdf_scratch_bytes_golden.py <path to that build's libgpsslam_hip.so>); tests/test_abi_cpu.py holds
the current library to it, because callers size per-view scratch buffers and saved state with this number."""
import ctypes
import json
import os
import sys

SIZES = [(640, 480), (1200, 680), (100, 75), (77, 50), (1, 1)]
TABLES = [(0x100000, 0x20000), (1 << 12, 64), (1 << 10, 1 << 9), (32, 1)]   # (n_buckets, n_excess); the first is the default

if __name__ == "__main__":
    lib = ctypes.CDLL(sys.argv[1])
    lib.gps_tsdf_scratch_bytes.restype = ctypes.c_int64
    lib.gps_tsdf_scratch_bytes.argtypes = [ctypes.c_int] * 4
    rows = [[w, h, nb, ne, int(lib.gps_tsdf_scratch_bytes(w, h, nb, ne))] for (w, h) in SIZES for (nb, ne) in TABLES]
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tsdf_scratch_bytes.json")
    with open(out, "w") as f:
        json.dump({"columns": ["width", "height", "n_buckets", "n_excess", "bytes"], "rows": rows}, f, indent=0)
        f.write("\n")
    print(out, len(rows))
