"""The C-ABI library loads (no GPU needed) and exports exactly what include/vrnet_hip.h declares."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_are_exported():
    import __graft_entry__ as g
    g.build()
    import asy_vrnet_amd.hip as hip
    text = open(os.path.join(ROOT, "include", "vrnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(vrnet_\w+)\s*\(", text))
    assert declared == set(hip.EXPORTED), declared ^ set(hip.EXPORTED)
    for name in declared:
        assert hasattr(hip._lib, name)
    assert hip._lib.vrnet_abi_version() == hip.ABI_VERSION


def test_no_oracle_import_in_product():
    pkg = os.path.join(ROOT, "asy-vrnet_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "oracle" not in src.replace("no oracle", ""), fn


def test_host_package_reads_only_the_library_path_from_the_environment():
    """Every os.environ / os.getenv use under asy-vrnet_amd/, with the variable it reads (None: not a string constant):
    the only one is VRNET_HIP_LIB in hip.py, which selects the library.  A stray variable in a user's shell changes nothing."""
    pkg = os.path.join(ROOT, "asy-vrnet_amd")
    reads = []
    for fn in sorted(os.listdir(pkg)):
        if not fn.endswith(".py"):
            continue
        tree = ast.parse(open(os.path.join(pkg, fn)).read(), fn)
        parent = {child: node for node in ast.walk(tree) for child in ast.iter_child_nodes(node)}
        for node in ast.walk(tree):
            if not (isinstance(node, ast.Attribute) and node.attr in ("environ", "getenv")
                    and isinstance(node.value, ast.Name) and node.value.id == "os"):
                continue
            use = parent[node]
            if isinstance(use, ast.Attribute):                     # os.environ.get(...)
                use = parent[use]
            name = use.args[0] if isinstance(use, ast.Call) and use.args else getattr(use, "slice", None)
            reads.append((fn, name.value if isinstance(name, ast.Constant) else None))
    assert reads == [("hip.py", "VRNET_HIP_LIB")], reads
