#!/usr/bin/env python3
"""Golden vectors of the reference's ``custom_softplus`` (EmbeddingModel.py:90-96) by EXECUTING it.

Like make_golden.py: runs only where the reference tree is present, imports it with tests/golden/tf_shim ahead of
it on sys.path.  The shim's ``tf.custom_gradient`` is inert, so the function returns ``(value, grad_fn)``: the value
and ``grad_fn(1)`` are recorded on a grid of x in [-90, 90], in float64 and in float32 (where 9999 e^x overflows from
x = 79.6 on: value inf, gradient 1).  This pins the 9999 and the form of the gradient.

Usage:  python tests/golden/make_golden_focuse.py         (writes tests/golden/focuse.npz — data only)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("EMGRAPH_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(HERE, "tf_shim"))

import numpy as np  # noqa: E402
import tensorflow as tf  # noqa: E402  (the shim)

assert tf.__version__.endswith("numpy-shim")

from emgraph.models.EmbeddingModel import custom_softplus  # noqa: E402


def main():
    x64 = np.concatenate([np.linspace(-90.0, 90.0, 361), np.array([-9.21, 0.0, 79.5, 79.7, 88.7, 88.8])])
    out = {"x": x64}
    with np.errstate(over="ignore"):
        for tag, x in (("f64", x64), ("f32", x64.astype(np.float32))):
            value, grad_fn = custom_softplus(x)
            out["value_" + tag] = np.asarray(value)
            out["grad_" + tag] = np.asarray(grad_fn(np.ones_like(x)))
    np.savez_compressed(os.path.join(HERE, "focuse.npz"), **out)
    print("wrote focuse.npz:", {k: (v.dtype.name, v.shape) for k, v in out.items()})


if __name__ == "__main__":
    main()
