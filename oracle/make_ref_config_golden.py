"""Commit the reference's experiment configurations as a test fixture.

TEST INFRASTRUCTURE ONLY.  Run where a checkout of the reference is available:

    python oracle/make_ref_config_golden.py <reference checkout>     # writes tests/golden/ref_configs.json.gz

The fixture holds the text of every configs/*.yaml of the reference, byte for byte, keyed by file name: the input data of
tests/test_config.py, which loads each one through core.config unmodified and compares it with the presets, so that the
suite does not need the reference tree.
"""
import glob
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "ref_configs.json.gz")


def main(ref):
    files = sorted(glob.glob(os.path.join(ref, "configs", "*.yaml")))
    assert files, "no configs/*.yaml under %s" % ref
    yamls = {}
    for f in files:
        with open(f, "rb") as fh:
            yamls[os.path.basename(f)] = fh.read().decode("utf-8")
    blob = json.dumps({"source": "configs/*.yaml of the reference", "yamls": yamls}, sort_keys=True).encode()
    with gzip.GzipFile(OUT, "wb", mtime=0) as fh:
        fh.write(blob)
    print("%s: %d configs" % (os.path.relpath(OUT), len(yamls)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
