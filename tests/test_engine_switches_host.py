"""The switch table of csrc/engine_switches.h against the environment rules it replaced, without a GPU: tests/host/switches_main.cpp
(its own main, the expected values written out row by row) is compiled with the host C++ compiler under the address and
undefined-behaviour sanitizers and run as a child process."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'nn-active-learning_amd', 'csrc')


def test_switch_table_keeps_every_legacy_parse_rule(tmp_path):
    cxx = os.environ.get('CXX') or shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'switches_main')
    # the sanitizer runtimes are linked statically (clang's default): the program then runs under whatever environment it is given
    static = [] if 'clang' in os.path.basename(cxx) else ['-static-libasan', '-static-libubsan']
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all'] + static + ['-I', CSRC, os.path.join(ROOT, 'tests', 'host', 'switches_main.cpp'), '-o', exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith('ALQ_')}      # the program sets the ALQ_* names itself
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r'engine switches ok: \d+ rows x 6 settings', r.stdout)


def test_table_lists_every_variable_the_documentation_does():
    """INTEGRATION.md's table and the header's name the same variables in the same order."""
    hdr = open(os.path.join(CSRC, 'engine_switches.h')).read()
    table = re.findall(r'ALQ_SW\("(ALQ_\w+)"', hdr)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    doc = doc[doc.index('### Engine switches'):]
    doc = doc[:doc.index('\n### ', 4)]
    rows = re.findall(r'^\| `(ALQ_\w+)` \|', doc, re.M)
    assert len(table) >= 40 and rows == table
