#!/usr/bin/env python
"""Prints the two constant tables of csrc/gm_shrot.hip: SHROT_DIR, the 32 Fibonacci sample directions rounded to float32 (a fourth, zero
column pads a row to 16 bytes), and SHROT_PINVT, the transposed pseudo-inverse (float64, then rounded) of the 32 x 16 matrix of gm_sh.h's
basis functions AT THOSE ROUNDED directions: row j holds the 16 weights of sample j.  Host only.
tests/test_sh_rotate_host.py holds the tables in the source file to this computation.
    python tools/sh_rotate_table.py"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import numpy as np
import sh_rotate_ref as ref

K = 32


def tables():
    D = ref.fibonacci_directions(K).astype(np.float32)
    P = np.linalg.pinv(ref.basis(D.astype(np.float64)))          # [16, K]
    return D, P.astype(np.float32), float(np.linalg.cond(ref.basis(D.astype(np.float64))))


def c_float(v):
    t = "%.9g" % v
    return (t if "." in t or "e" in t else t + ".0") + "f"


def c_rows(a):
    return ",\n".join("    {" + ", ".join(c_float(v) for v in row) + "}" for row in a)


if __name__ == "__main__":
    D, P, cond = tables()
    print("// %d Fibonacci directions; condition number of the basis matrix %.3f" % (K, cond))
    print("__constant__ float SHROT_DIR[%d][4] = {\n%s};" % (K, c_rows(np.concatenate([D, np.zeros((K, 1), np.float32)], 1))))
    print("__constant__ float SHROT_PINVT[%d][16] = {\n%s};" % (K, c_rows(P.T)))
