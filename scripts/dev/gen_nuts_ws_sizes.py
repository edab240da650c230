"""Write tests/golden/nuts_ws_sizes.json: the NUTS workspace sizes of the library that HMC_AMD_LIB
names (default: the tree's own), over the grid of tests/test_abi.py::test_nuts_workspace_sizes_golden.
Host-only queries, no GPU.  The committed file came from the library built at the commit before the
layouts moved into csrc/hmc_nuts_layout.hpp:

    HMC_AMD_LIB=<that commit's libhmc.so> python scripts/dev/gen_nuts_ws_sizes.py
"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "understanding-hmc_amd"))

NS = (0, 1, 15, 16, 17, 1000, 16385)          # 16385 crosses the lockstep kernel's 1024-block cap
DMAX = (1, 10, 30)
NUTS_D = (1, 16, 17, 32, 33, 64, 65, 112, 113, 128, 129, 192, 193, 320, 321, 500)
ITERS = (1, 32, 33)
GLM_D = (1, 16, 17, 33, 65, 128)


def main():
    from hmc_amd import _lib as H
    L = H.lib()
    nuts = [[D, n, d, it, pm, L.hmc_nuts_workspace_size_ex(D, n, d, it, pm)]
            for D, n, d, it, pm in itertools.product(NUTS_D, NS, DMAX, ITERS, (0, 1))]
    glm = [[D, n, d, L.hmc_glm_nuts_workspace_size(D, n, d)] for D, n, d in itertools.product(GLM_D, NS, DMAX)]
    out = os.path.join(ROOT, "tests", "golden", "nuts_ws_sizes.json")
    with open(out, "w") as f:
        json.dump({"nuts_columns": ["D", "n", "d_max", "iters", "pm", "bytes"], "nuts": nuts,
                   "glm_columns": ["D", "n", "d_max", "bytes"], "glm": glm}, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d + %d entries from %s" % (out, len(nuts), len(glm), H.LIB_PATH))


if __name__ == "__main__":
    main()
