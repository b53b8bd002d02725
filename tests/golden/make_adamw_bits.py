"""Records tests/golden/adamw_bits.npz: the bits of fsr_adamw_step / fsr_adamw_step_scaled on the MI355X.

Run ONCE, on the GPU, against a library built from the commit BEFORE the AdamW kernels were merged into one template (its scalar
adamw_kernel / adamw_scaled_kernel are the reference the fixture exists to keep):

    FSR_HIP_LIB=<that build's libfsr_hip.so> python tests/golden/make_adamw_bits.py [--out tests/golden/adamw_bits.npz]

Re-recording from a current build would only pin the kernel to itself.  The cases, the hyper-parameters and the replay are those of
tests/test_adamw_bits.py (imported, not restated); the inputs are optim_contract.adam_inputs, stored so that the test does not depend
on torch's CPU generator."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository root

import optim_contract as C
import test_adamw_bits as T


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.FIXTURE)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("make_adamw_bits.py records on the MI355X; no GPU here")
    dev = torch.device("cuda:0")
    out = {}
    for count, step0, wd, scaled, offset in T.CASES:
        inputs = C.adam_inputs(step0, count)
        for k, x in zip("pgmv", inputs):
            out[T.in_key(count, step0) + k] = np.ascontiguousarray(x, dtype=np.float32)
        got = T.replay(dev, inputs + (step0,), wd, scaled, offset, "value")
        for name, t in zip(("p", "m", "v", "step"), got):
            out[T.out_key(count, step0, wd, scaled, offset) + name] = t.numpy().copy()
    np.savez(a.out, **out)
    print("%s: %d cases from %s, %d bytes" % (a.out, len(T.CASES), T.L.LIB_PATH, os.path.getsize(a.out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
