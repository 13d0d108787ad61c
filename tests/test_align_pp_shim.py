"""The level-0 hmmalign executable with PP: the C client against a resident Server(GpuBackend) on golden pairs, its
Stockholm file against hmmalign's stored one (tests/golden/align_pp) - every line equal, PP characters one step apart at
most and only inside the guard band of the float32 tolerance."""
import os
import subprocess
import threading

import numpy as np
import pytest

from tests import pp_reference as ppr
from tests.conftest import load_case
from tests.test_align_pp import BOUNDS, _need_gpu, _steps, tol32

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "witch_amd", "shim", "bin")


@pytest.mark.parametrize("name,queries,models", [("dna_hmmbuild", (0, 7, 23), (0, 5)), ("amino_hmmbuild", (1, 30), (2,))])
def test_hmmalign_client_writes_hmmalign_files(name, queries, models, tmp_path):
    _need_gpu()
    import shutil
    import tempfile
    from witch_amd.shim.server import GpuBackend, Server
    case = load_case(name)
    ref = {(r[0], r[1]): r for r in ppr.case_reference(name)}
    stored = {(p["q"], p["h"]): p["sto"] for p in ppr.load_fixture(name)["pairs"]}
    d = tempfile.mkdtemp(prefix="wh_sock_", dir="/tmp")
    try:
        sock = os.path.join(d, "s.sock")
        srv = Server(GpuBackend(0), sock)
        ready = threading.Event()
        threading.Thread(target=srv.serve_forever, args=(ready,), daemon=True).start()
        assert ready.wait(10)
        env = dict(os.environ, WITCH_HIP_SOCKET=sock)
        jobs = [(q, h) for q in queries for h in models]
        for q, h in jobs:
            fa = tmp_path / ("q%d.fa" % q)
            fa.write_text(">%s\n%s\n" % (case.qnames[q], case.qseqs[q]))
        # all at once: the server batches them into one launch and must hand every client its own slice
        procs = [subprocess.Popen([os.path.join(BIN, "hmmalign"), "-o", str(tmp_path / ("o_%d_%d.sto" % (q, h))), case.hmm_paths[h],
                                   str(tmp_path / ("q%d.fa" % q))], env=env) for q, h in jobs]
        assert all(p.wait(120) == 0 for p in procs)
        for q, h in jobs:
            got = (tmp_path / ("o_%d_%d.sto" % (q, h))).read_text().splitlines()
            want = stored[(q, h)].splitlines()
            assert len(got) == len(want), (q, h)
            _, _, cols, digits, post = ref[(q, h)]
            band = np.min(np.abs(post[:, None] - BOUNDS[None, :]), axis=1) <= tol32(len(post))
            for a, b in zip(got, want):
                if a == b:
                    continue
                assert a.startswith(("#=GR", "#=GC PP_cons")) and len(a) == len(b), (q, h, a, b)
            g = ppr.parse_stockholm("\n".join(got))
            w = ppr.parse_stockholm("\n".join(want))
            assert g[0] == w[0] and g[1] == w[1] and g[4] == w[4]
            gd = ppr.row_cols_digits(g[1], g[2], g[4])[1]
            for i, (x, y) in enumerate(zip(gd, digits)):
                assert x == y or (band[i] and _steps(x, y) == 1), (q, h, i, x, y)
    finally:
        shutil.rmtree(d, ignore_errors=True)
