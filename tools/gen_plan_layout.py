"""Records tests/golden/plan_layout.json: everything the plan table and the
chain-set builder (csrc/plans.hip, chain_set.h) decide on the host, read
through the C ABI's size queries of every plan (2 nets x 4 precisions).  No
device is needed.  tests/test_plan_layout.py asserts exact equality with the
fixture, so record it from a build whose layout is known good BEFORE changing
the host code, never from the build under test:

  python tools/gen_plan_layout.py                      # the in-tree library
  CODENERF_MEASURE=1 python tools/gen_plan_layout.py --lib other/libcodenerf_hip.so
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "plan_layout.json")
NETS = ((3, 1), (2, 1))
PRECISIONS = (0, 1, 2, 3)            # CN_FP32, CN_BF16, CN_BF16X3, CN_BF16X3F
SAMPLES = (1, 256, 257, 4133)        # one tile, a full tile, one over, ragged
PLANE_KINDS = range(7)               # CN_PLANE_* of include/codenerf.h
PLANE_INDICES = range(12)


def record(lib):
    """{"sb_tb_precision": {query: value}} of every plan of a typed library."""
    out = {}
    for sb, tb in NETS:
        for prec in PRECISIONS:
            h = ctypes.c_void_p()
            if lib.cn_plan_create(sb, tb, 256, 10, 4, 256, prec, ctypes.byref(h)) != 0:
                raise RuntimeError(lib.cn_last_error().decode())
            plan = {
                "num_params": lib.cn_plan_num_params(h),
                "num_inject": lib.cn_plan_num_inject(h),
                "blob_floats": lib.cn_blob_floats(h),
                "packed_bytes": [lib.cn_packed_bytes(h, 0), lib.cn_packed_bytes(h, 1)],
                "act_bytes_per_sample": lib.cn_act_bytes_per_sample(h),
                "samples": {},
            }
            for M in SAMPLES:
                planes = []
                for kind in PLANE_KINDS:
                    for index in PLANE_INDICES:
                        w = ctypes.c_int(-1)
                        planes.append([lib.cn_act_plane(h, M, kind, index, ctypes.byref(w)), w.value])
                plan["samples"][str(M)] = {
                    "pad_samples": lib.cn_pad_samples(h, M),
                    "act_bytes": lib.cn_act_bytes(h, M),
                    "dw_ws_bytes": lib.cn_dw_ws_bytes(h, M),
                    "planes": planes,            # [offset, width], kind-major
                }
            lib.cn_plan_destroy(h)
            out[f"{sb}_{tb}_{prec}"] = plan
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="library to record from (default: the in-tree build)")
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    import codenerf_amd._lib as L
    data = record(L.load_library(a.lib or L.LIB_PATH))
    with open(a.out, "w") as f:
        json.dump(data, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"wrote {a.out}: {len(data)} plans")
