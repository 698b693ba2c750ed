"""The harness of the host-side geometry checks: tests/<name>_geo_check.cpp walks a launcher's geometry
header (csrc/*_geo.hpp) as a stand-alone program under ASan and UBSan and prints one JSON line per shape.
`compile_check` builds such a program, `run_check` gives the lines of shapes whose walks must pass, and
`run_raw` the finished process of a run that the test judges itself (the shapes the geometry must refuse)."""
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'baseband-tasks_amd', 'csrc')
PIPES = dict(stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def compile_check(name, where, opt='-O1'):
    """tests/<name>.cpp as a stand-alone program under ASan and UBSan; its path."""
    exe = os.path.join(str(where), name)
    subprocess.check_call(['g++', opt, '-g', '-std=c++17', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', '-I', CSRC,
                           os.path.join(ROOT, 'tests', name + '.cpp'), '-o', exe])
    return exe


def _words(shape):
    """A shape as the program's arguments: integers, and strings (a float in hex, say) as they are."""
    return [v if isinstance(v, str) else str(int(v)) for v in shape]


def run_raw(exe, shapes, word=None):
    """The finished process (stdout, stderr, returncode) of the program on `shapes`, tuples or one string of
    arguments, behind the leading `word` if the program takes one.  Nothing is asserted."""
    args = shapes.split() if isinstance(shapes, str) else [w for shape in shapes for w in _words(shape)]
    return subprocess.run([exe] + ([word] if word else []) + args, **PIPES)


def run_check(exe, shapes, through_stdin=False, word=None):
    """The program's JSON line for each of `shapes` (tuples), given as arguments or, a long list, on the
    standard input of four copies of the program, a quarter each; the walks must pass."""
    if through_stdin:
        lines = [' '.join(_words(shape)) for shape in shapes]
        step = -(-len(lines) // 4)
        with ThreadPoolExecutor(4) as pool:
            outs = list(pool.map(lambda start: subprocess.run([exe], input='\n'.join(lines[start:start + step]), **PIPES),
                                 range(0, len(lines), step)))
    else:
        outs = [run_raw(exe, shapes, word)]
    done = [(out.stdout, out.stderr, out.returncode) for out in outs]
    for stdout, stderr, code in done:
        assert code == 0, stdout[-2000:] + stderr[-4000:]
    plans = [json.loads(line) for stdout, _, _ in done for line in stdout.splitlines()]
    assert len(plans) == len(shapes)
    return plans
