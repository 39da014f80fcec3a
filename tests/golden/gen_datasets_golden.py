"""Writes tests/golden/datasets_reference_items.npz for tests/test_datasets_cpu.py: the items the upstream project's own
loaders (datasets/scanobjectnn.py, datasets/s3dis_v2.py) return on the test's synthetic files.

    python tests/golden/gen_datasets_golden.py <upstream checkout>"""
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import test_datasets_cpu as T      # noqa: E402


def main(ref_dir):
    d = tempfile.mkdtemp()
    try:
        T.make_files(d)
        shutil.copy(T.run_side("ref", d, ref=ref_dir), T.GOLDEN)
    finally:
        shutil.rmtree(d)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
