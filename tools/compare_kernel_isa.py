"""Compare the kernels two builds of one HIP source share: resource usage and instruction streams.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Rpass-analysis=kernel-resource-usage --save-temps -c X.hip   (once per build, each in a
    directory of its own, stderr kept as remarks.txt)
    python tools/compare_kernel_isa.py OLD_DIR NEW_DIR [name filter ...]

Kernels are matched by their demangled names without the parameter list (an empty trailing parameter pack leaves the name as it was).
For every pair it prints the resource-usage remarks of both builds and whether the instruction streams are identical (labels,
comments and symbol names normalised).  Used for profiles/pcm_device.md."""
import glob
import re
import shutil
import subprocess
import sys


def remarks(path):
    out, name = {}, None
    for ln in open(path):
        if 'remark:' not in ln:
            continue
        body = ln.split('remark:', 1)[1].split('[-Rpass')[0].strip()
        body = re.sub(r'^\S+:\d+:\d+:\s*', '', body)
        if body.startswith('Function Name:'):
            name = body.split(':', 1)[1].strip()
            out[name] = []
        elif name and ':' in body:
            out[name].append(body)
    return out


def bodies(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)^\s*s_endpgm', txt, re.S | re.M):
        lines = []
        for ln in m.group(2).splitlines():
            ln = ln.split(';')[0].strip()
            if not ln or ln.startswith('.') or ln.endswith(':'):
                continue
            lines.append(re.sub(r'_Z\w+', 'SYM', re.sub(r'\.LBB\d+_\d+', 'L', ln)))
        out[m.group(1)] = lines
    return out


def demangle(names):
    r = subprocess.run([shutil.which('c++filt') or shutil.which('llvm-cxxfilt') or 'c++filt'], input='\n'.join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.splitlines()))


def key(dem):
    """the demangled name with its template arguments, without return type and parameter list"""
    d = dem.split('(')[0].replace('void ', '').replace('vr::', '')
    return d


def main():
    old_dir, new_dir = sys.argv[1:3]
    filt = sys.argv[3:] or ['stft_tile_kernel', 'istft_tile_kernel']
    sides = []
    for d in (old_dir, new_dir):
        asm = bodies(glob.glob(d + '/*gfx950*.s')[0])
        rem = remarks(d + '/remarks.txt')
        dem = demangle(list(asm))
        sides.append({key(dem[k]): (k, asm[k], rem.get(k, [])) for k in asm if any(f in dem[k] for f in filt)})
    old, new = sides
    for k in sorted(set(old) | set(new)):
        if k not in old:
            print('NEW   %s\n      %s' % (k, '; '.join(new[k][2])))
            continue
        if k not in new:
            print('GONE  %s' % k)
            continue
        same_isa = old[k][1] == new[k][1]
        same_res = old[k][2] == new[k][2]
        print('%s %s\n      resources %s: %s\n      instructions: %d vs %d, %s' % (
            'SAME ' if same_isa and same_res else 'DIFF ', k, 'identical' if same_res else 'DIFFER', '; '.join(new[k][2]),
            len(old[k][1]), len(new[k][1]), 'identical' if same_isa else 'DIFFERENT'))
        if not same_res:
            print('      old: %s' % '; '.join(old[k][2]))


if __name__ == '__main__':
    main()
