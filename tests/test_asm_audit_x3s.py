"""Build-time audit of conv_x3s.hip, as tests/test_asm_audit.py does it for conv_x3h.hip / conv_x3d.hip: the stride-2 kernel keeps the
dwordx2 pixel loads of two chunks in flight across hand-placed `s_waitcnt vmcnt(N)`, so nothing between a load and the wait that covers
it may read, copy or overwrite its register pair.  tools/asm_inflight_audit.py follows the vmcnt arithmetic, tools/asm_inflight_audit2.py
the registers by name (x3s_wait8 lists the pairs it releases in a `; landed` comment): both must report nothing for every
`conv_x3h_kernel_s2` instantiation.  No GPU: hipcc cross-compiles to assembly (~1 min)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'vocal-remover_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
AUDIT = os.path.join(ROOT, 'tools', 'asm_inflight_audit.py')
AUDIT2 = os.path.join(ROOT, 'tools', 'asm_inflight_audit2.py')
INSTANCES = 2                      # <64, 8> and <32, 8>


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_no_instruction_touches_an_in_flight_pixel_pair(tmp_path):
    asm = str(tmp_path / 'conv_x3s.s')
    r = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-S', '--cuda-device-only', '-o', asm,
                        os.path.join(CSRC, 'conv_x3s.hip')], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([sys.executable, AUDIT, asm, 'conv_x3h_kernel_s2'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln for ln in r.stdout.splitlines() if ln.rstrip().endswith('violations') and ' register loads, ' in ln]
    assert len(rows) == INSTANCES, r.stdout[-2000:]
    for ln in rows:
        loads, bad = int(ln.split(': ', 1)[1].split(' register loads, ')[0]), int(ln.split(' register loads, ')[1].split(' ')[0])
        # (prologue 4 + 2 x 24, the two unrolled chunk bodies 24 each: 100 pair loads at least)
        assert loads >= 100 and bad == 0, (ln, r.stdout[-2000:])
    r = subprocess.run([sys.executable, AUDIT2, asm, 'conv_x3h_kernel_s2'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.count(' 0 reports') == INSTANCES, r.stdout[-2000:]
    for ln in r.stdout.splitlines():
        if ' asm loads, ' in ln:
            # the waits must be there to be followed: 3 register sets x (prologue + two chunk bodies) + the epilogue constants
            assert int(ln.split(' asm loads, ')[1].split(' waits')[0]) >= 10, ln
