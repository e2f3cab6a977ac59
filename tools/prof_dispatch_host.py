"""Host time of the kernel selection alone: SDFNetwork.eval_points and EnvmapMaterialNetwork.forward on the CPU with every `ops` function and
packer stubbed out (the recorder of tools/gen_dispatch_golden.py with its bookkeeping removed), so what is timed is the Python between the
caller and the kernels.  Runs unchanged before and after a change of the selection code; five repeats, microseconds of process CPU time per call (wall-clock time on a shared machine measures the neighbours).

    python tools/prof_dispatch_host.py [calls per repeat, default 20000]
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_dispatch_golden as gen  # noqa: E402


class Stubs(gen.Recorder):
    def _op(self, name, real):
        n_out = gen.N_RESULTS.get(name, 1)
        out = gen.Fake() if n_out == 1 else tuple(gen.Fake() for _ in range(n_out))
        return lambda *a, **k: out


def main(calls):
    torch.set_num_threads(1)
    m = gen.build_nets()
    x = torch.zeros(5, 3)
    noise = {"spec": torch.zeros(5, 32), "normal": torch.zeros(5, 60)}
    shapes = {"eval_points(full, grad)": lambda: m["sdf"].eval_points(x, 2.0, 0.5, full=True, grad=True),
              "eval_points(sdf only)": lambda: m["sdf"].eval_points(x, 2.0, 0.5, full=False),
              "EnvmapMaterialNetwork.forward": lambda: m["material"](x, noise=noise)}
    with Stubs():
        for name, fn in shapes.items():
            fn()
            us = []
            for _ in range(5):
                t0 = time.process_time()
                for _ in range(calls):
                    fn()
                us.append((time.process_time() - t0) / calls * 1e6)
            print(f"{name}: median {statistics.median(us):.2f} us per call (five repeats of {calls}: " + ", ".join(f"{u:.2f}" for u in us) + ")")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20000)
