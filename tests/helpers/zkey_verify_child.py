"""Child process of tests/test_gpu_zkey_verify.py: zkp_amd.zkey_verify_frominit of the key files
argv[3:] against the initial key argv[1] with the seed argv[2] (hex), under whatever
ZKP_VERIFY_CHUNK the parent set for this process.  Prints one JSON line: per key [valid, message],
or {"status": zkp_status} where the call failed."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zk-p2p-onramp_amd"))

import zkp_amd  # noqa: E402


def main():
    init = open(sys.argv[1], "rb").read()
    seed = bytes.fromhex(sys.argv[2])
    out = []
    for path in sys.argv[3:]:
        try:
            out.append(list(zkp_amd.zkey_verify_frominit(init, open(path, "rb").read(), seed=seed)))
        except zkp_amd.ZkpError as e:
            out.append({"status": e.status})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
