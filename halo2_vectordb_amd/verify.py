"""The Verify arm on the command line (the reference's SnarkCmd::Verify, src/scaffold/mod.rs:298-320):

    python -m halo2_vectordb_amd.verify proof.snark key.vk [tau]
    python -m halo2_vectordb_amd.verify proof.snark key.vk --params kzg_bn254_k.srs

proof.snark: io.write_snark's file; key.vk: ProverRounds.save_verifying_key's .npz or halo2's RawBytes key (save_verifying_key_raw;
tau: the SRS scalar, the reference's gen_srs scalar by default; --params: the halo2 params file the proof's SRS came from, whose
g2 and [tau]_2 the pairing takes — for either kind of key).  Prints {"accepted": ..., "verify_s": ...} and exits 0 when the
proof is accepted, 1 otherwise (a malformed file included).  verify_s is the reading of both files and the verification; binding
the GPU (the HIP runtime's start-up, about a second in a fresh process) comes before it and is reported as init_s."""
import json
import sys
import time


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    params = None
    if "--params" in argv:
        at = argv.index("--params")
        if at + 1 >= len(argv):
            print(__doc__, file=sys.stderr)
            return 2
        params = argv[at + 1]
        argv = argv[:at] + argv[at + 2:]
    if len(argv) not in (2, 3) or (params is not None and len(argv) != 2):
        print(__doc__, file=sys.stderr)
        return 2
    from . import _lib
    from .verifier import Verifier
    t0 = time.perf_counter()
    _lib.init()
    init_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    try:
        v = Verifier.from_files(argv[0], argv[1], tau=int(argv[2], 0) if len(argv) == 3 else None, params=params)
        ok, timings = v.verify(), v.timings
    except (OSError, ValueError) as e:
        ok, timings = False, {"error": str(e)}
    print(json.dumps({"accepted": bool(ok), "verify_s": round(time.perf_counter() - t0, 4), "init_s": round(init_s, 4),
                      "stages_s": {k: (round(s, 4) if isinstance(s, float) else s) for k, s in timings.items()}}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
