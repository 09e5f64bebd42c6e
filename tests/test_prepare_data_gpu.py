"""GPU: python -m stylerenderer_amd.prepare_data --gpu 0 writes the store that --gpu -1 writes, file for file."""
import os

import pytest

from prepare_data_cases import make_folder
from stylerenderer_amd import prepare_data

pytest.importorskip("PIL")
pytestmark = pytest.mark.gpu


def read_all(path):
    return {name: open(os.path.join(path, name), "rb").read() for name in sorted(os.listdir(path))}


@pytest.mark.parametrize("fmt", ["jpeg", "npy"])
def test_device_store_equals_host_store(tmp_path, fmt):
    src = str(tmp_path / "src")
    good = make_folder(src)
    for gpu, out in (("0", "dev"), ("-1", "host")):
        assert prepare_data.main(["--out", str(tmp_path / out), "--size", "16,32,64", "--format", fmt, "--gpu", gpu,
                                  "--n_worker", "4", src]) == 0
    dev, host = read_all(str(tmp_path / "dev")), read_all(str(tmp_path / "host"))
    assert len(host) == 3 * len(good) + 1
    assert sorted(dev) == sorted(host)
    for name in host:
        assert dev[name] == host[name], name
