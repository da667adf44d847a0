#!/usr/bin/env python3
"""Host wall-clock of aq_prepare_data_bed (PLINK .bed blocks, 2 bits per genotype, unpacked on the GPU) against
aq_prepare_data on the same dosages as int8 -- the path that existed before, the yardstick -- in one process, at the X of
bench.py's shape (n = 1000, p = 50 000 unless AQ_BENCH_N/P say otherwise; q = 8 traits, no missing call).  One warm-up
call, then three timed calls each, the clock around the C call (upload, decode, column statistics, hashes, compact
standardise, centring of Y; the handle is destroyed outside the clock).  Prints one JSON line with the bytes uploaded
(DESIGN.md section 9, N1).  The decode kernel alone is read off a kernel trace of this tool:

    python tools/time_prepare_bed.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_prepare_bed.py      # aq_k_bed_decode in the kernel stats
"""
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_fileset(prefix, G):
    """A1 dosages 0 / 1 / 2 (n x p) as prefix.bed / .bim / .fam: code 0 = hom A1, 2 = het, 3 = hom A2, four per byte."""
    n, p = G.shape
    stride = (n + 3) // 4
    codes = np.zeros((4 * stride, p), dtype=np.uint8)
    codes[:n] = np.array([3, 2, 0], dtype=np.uint8)[G]
    quad = codes.reshape(stride, 4, p)
    blocks = quad[:, 0] | (quad[:, 1] << 2) | (quad[:, 2] << 4) | (quad[:, 3] << 6)
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(np.ascontiguousarray(blocks.T).tobytes())
    with open(prefix + ".bim", "w") as f:
        f.writelines(f"1\trs{j + 1}\t0\t{j + 1}\tA\tG\n" for j in range(p))
    with open(prefix + ".fam", "w") as f:
        f.writelines(f"f{i + 1} i{i + 1} 0 0 0 -9\n" for i in range(n))


def main():
    from atlasqtl_amd import PlinkBed, _lib
    n, p = (int(os.environ.get(k, d)) for k, d in (("AQ_BENCH_N", 1000), ("AQ_BENCH_P", 50000)))
    q = 8
    rng = np.random.default_rng(1)
    G = np.asfortranarray(rng.binomial(2, rng.uniform(0.05, 0.5, size=p)[None, :], size=(n, p)).astype(np.int8))
    Y = np.asfortranarray(rng.normal(size=(n, q)))
    L = _lib.lib()
    with tempfile.TemporaryDirectory() as tmp:
        write_fileset(os.path.join(tmp, "x"), G)
        bed = PlinkBed(os.path.join(tmp, "x"))
        blocks = bed.packed()                                    # the memory map: the first upload also reads the file

        def run_bed():
            pin = _lib.AqPrepBedInput()
            pin.n_file, pin.n, pin.p, pin.q = n, n, p, q
            pin.bed, pin.sample_idx, pin.Y = C.cast(blocks.ctypes.data, C.POINTER(C.c_uint8)), None, _lib.as_dp(Y)
            pin.count_a2, pin.missing, pin.device = 0, 0, 0
            h = C.c_void_p()
            t = time.perf_counter()
            rc = L.aq_prepare_data_bed(C.byref(pin), C.byref(h))
            dt = time.perf_counter() - t
            _lib.check(rc, "aq_prepare_data_bed")
            return dt, h

        def run_i8():
            pin = _lib.AqPrepInput()
            pin.n, pin.p, pin.q, pin.X, pin.X_i8, pin.Y, pin.device = n, p, q, None, G.ctypes.data_as(C.POINTER(C.c_int8)), _lib.as_dp(Y), 0
            h = C.c_void_p()
            t = time.perf_counter()
            rc = L.aq_prepare_data(C.byref(pin), C.byref(h))
            dt = time.perf_counter() - t
            _lib.check(rc, "aq_prepare_data")
            return dt, h

        def timed(fn):
            out, kept = [], None
            for it in range(4):                                  # the first call is the warm-up
                dt, h = fn()
                if it:
                    out.append(round(dt, 5))
                pk = C.c_int32(0)
                _lib.check(L.aq_prep_info(h, C.byref(pk), None, None, None, None, None), "aq_prep_info")
                kept = int(pk.value)
                L.aq_prep_destroy(h)
            return out, kept

        t_i8, kept_i8 = timed(run_i8)
        t_bed, kept_bed = timed(run_bed)
        assert kept_i8 == kept_bed
        print(json.dumps(dict(n=n, p=p, q=q, p_kept=kept_bed, prepare_data_int8_s=t_i8, prepare_data_bed_s=t_bed,
                              upload_bytes_int8=n * p, upload_bytes_bed=p * bed.stride,
                              decode_bytes_in=p * bed.stride, decode_bytes_out=n * p)))
        del blocks, bed


if __name__ == "__main__":
    main()
