"""The layering of ``smdt_amd.parallel``: dense <- feature modules <- tensor_parallel, imports
pointing downward only, and the weight-cache registry of ``dense``."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOWER = ["dense", "fp8_linear", "decode_weights", "moe_experts", "lm_head"]


@pytest.mark.parametrize("first", LOWER + ["tensor_parallel"])
def test_module_imports_first_and_stays_below_tensor_parallel(first):
    """Each module imports on its own in a fresh interpreter (an import cycle may bite in one import
    order only), and none of the five lower ones pulls in tensor_parallel."""
    code = (f"import sys, smdt_amd.parallel.{first}; "
            "print('smdt_amd.parallel.tensor_parallel' in sys.modules)")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == str(first == "tensor_parallel")


def test_registered_weight_cache_is_dropped(monkeypatch):
    from smdt_amd.parallel import dense
    monkeypatch.setattr(dense, "_WEIGHT_CACHES", list(dense._WEIGHT_CACHES))    # leave the registry as it was
    cache, dropped = {}, []
    p, other = torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(2))
    dense.register_weight_cache(cache.clear, lambda q: dropped.append(q) or cache.pop(id(q), None))
    cache[id(p)], cache[id(other)] = "p", "other"
    epoch = dense.WEIGHTS_EPOCH[0]
    dense.drop_cached_weight_t([p, other][:1])
    assert len(dropped) == 1 and dropped[0] is p and list(cache) == [id(other)]
    dense.drop_cached_weight_t([p, other])
    assert dense.WEIGHTS_EPOCH[0] == epoch + 2      # once per call, not once per parameter
    cache[id(p)] = "p"
    dense.params_changed()
    assert not cache and dense.WEIGHTS_EPOCH[0] == epoch + 3
