"""Which translation unit of halo2_vectordb_amd/csrc can reach the witness call's context (g_winv, gadgets.hpp): witness.hip alone.
The value-only code of the committed tree and index (resident.hip), the layout stage (layout.hip) and the hash-only Poseidon kernels
(poseidon.hip) do not include gadgets.hpp, and no kernel that takes the call's Streams is defined outside witness.hip."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2_vectordb_amd", "csrc")


def closure(name):
    """base names of the local files `name` includes, transitively (profiles/srchash.py's include closure)"""
    sys.modules.pop("srchash", None)
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import srchash
    seen = set()
    srchash._closure(os.path.join(CSRC, name), [CSRC, os.path.join(ROOT, "include")], seen)
    return {os.path.basename(f) for f in seen}


def test_only_witness_hip_includes_the_call_context():
    for name in ("resident.hip", "layout.hip", "poseidon.hip"):
        assert "gadgets.hpp" not in closure(name), name
        assert "common.hpp" in closure(name), name       # the closure does follow includes
    assert "gadgets.hpp" in closure("witness.hip")


def test_kernels_that_take_streams_are_witness_hips():
    kernel = re.compile(r"__global__\s+(?:__launch_bounds__\s*\([^)]*\)\s*)?(?:static\s+)?void\s+(\w+)\s*\(([^)]*)\)")
    found = {}
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".hpp", ".inc", ".cpp")):
            continue
        for m in kernel.finditer(open(os.path.join(CSRC, name), errors="replace").read()):
            if re.search(r"\bStreams\b", m.group(2)):
                found.setdefault(name, []).append(m.group(1))
    assert list(found) == ["witness.hip"], found
    assert {"k_dist_head", "k_mk_leaf_trace", "k_mku_level_trace", "k_mko_index"} <= set(found["witness.hip"])
