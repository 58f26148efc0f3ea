#!/usr/bin/env python3
"""pmc_subset.tar.xz: the bundled PMC corpus files the corpus-walk tests read, stored unmodified, so that
those tests run from a checkout alone.

    python tests/golden/make_pmc_subset.py <PMC corpus directory>

The archive holds the 50 files whose chunk hashes chunker.json and config1.json pin (two of them are not
UTF-8 and take the latin-1 fallback) and the first six files of the sorted corpus walk (tests/test_tokenizer.py).
Members are written in sorted order with zeroed owner and time stamps, so the archive is byte-stable."""
import io
import json
import os
import sys
import tarfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pmc_subset.tar.xz")


def main(pmc_dir: str) -> None:
    pinned = set(json.load(open(os.path.join(HERE, "chunker.json")))["sha256"])
    assert pinned == set(json.load(open(os.path.join(HERE, "config1.json")))["files"])
    head = sorted(f for f in os.listdir(pmc_dir) if f.startswith("PMC") and f.endswith(".txt"))[:6]
    with tarfile.open(OUT, "w:xz", format=tarfile.USTAR_FORMAT) as tf:
        for name in sorted(pinned | set(head)):
            data = open(os.path.join(pmc_dir, name), "rb").read()
            info = tarfile.TarInfo(name)
            info.size, info.mode, info.mtime = len(data), 0o644, 0
            tf.addfile(info, io.BytesIO(data))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
