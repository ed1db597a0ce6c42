"""The reference's UNCHANGED application sources, compiled against include/ + libgraphmat_hip.so (test infrastructure).

src/{PageRank,BFS,SGD,SSSP,IncrementalPageRank,TopologicalSort,DeltaStepping}.cpp of the reference tree are compiled where
they lie -- nothing of the reference is copied into the repository -- into oracle/_ref/ (git-ignored).  The reference tree
exists where the project is built, not necessarily where it is tested: the binaries travel with the tree, and the drop-in
tests (tests/test_dropin_apps.py, tests/test_gpu_multirank_apps.py) run whatever was built here.  GRAPHMAT_REFERENCE names
the reference tree.
"""
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
REF = os.environ.get("GRAPHMAT_REFERENCE", "/root/reference")
APPS = ("PageRank", "BFS", "SGD", "SSSP", "IncrementalPageRank", "TopologicalSort", "DeltaStepping")


def present():
    """True when the reference tree is here to be compiled."""
    return os.path.isdir(os.path.join(REF, "src"))


def path(name):
    """Where the binary of one application lies (whether or not it was built)."""
    return os.path.join(OUT, name)


def work():
    """(source, binary, extra flags) of every reference application; empty without the reference tree."""
    if not present():
        return []
    os.makedirs(OUT, exist_ok=True)
    w = [(os.path.join(REF, "src", app + ".cpp"), path(app), ()) for app in APPS]
    # the reference's own tracing build (-D__TIMING, its Makefile's `timing` flavour): per-iteration lines
    w.append((os.path.join(REF, "src", "PageRank.cpp"), path("PageRank__TIMING"), ("-D__TIMING",)))
    return w
