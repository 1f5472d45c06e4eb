"""Child of tests/test_table_exact.py's one-row-per-lane test -- started by subprocess from the pytest process (never an exec from a
process that holds the GPU), like tests/gpu_dual_worker.py.  The parent sets SYMPA_TABLE_GENERIC=1, which the library reads once per
process: egrad2rgrad and the tangent norm of dims 7..16 then run the one-row-per-lane kernels.

    gpu_table_worker.py <out.npz>      every case of tests/golden/exact_table_{upper,bounded}_n{7..16}.npz through ops.egrad2rgrad
                                       and ops.tangent_sqnorm; the results are saved for the parent to compare with the exact values
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    assert os.environ.get("SYMPA_TABLE_GENERIC") == "1", "the parent selects the one-row-per-lane kernels"
    from sympa_amd import ops
    dev = torch.device("cuda", 0)
    out = {}
    for model in ("upper", "bounded"):
        for n in range(7, 17):
            with np.load(os.path.join(ROOT, "tests", "golden", f"exact_table_{model}_n{n}.npz")) as f:
                for case in f["case_names"]:
                    z, g, x, u = (torch.from_numpy(f[f"{case}__{k}"]).to(dev) for k in ("z", "g", "x", "u"))
                    if case == "nonsym":       # a table row is symmetric: only projx takes the stored row
                        z = 0.5 * (z + z.transpose(-1, -2))
                    out[f"{model}_{n}_{case}_rgrad"] = ops.egrad2rgrad(z, g, model).cpu().numpy()
                    out[f"{model}_{n}_{case}_inner"] = ops.tangent_sqnorm(x, u, model).cpu().numpy()
            torch.cuda.synchronize()
            ops.check_status(dev)
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
