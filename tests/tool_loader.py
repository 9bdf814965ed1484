"""`tools/<name>.py` imported as a module by its file path, for the tests of the tools' arguments and helpers.  A plain
module, imported by the test files (tools/ is no package and is not on `sys.path`)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tool(name):
    spec = importlib.util.spec_from_file_location(f"tools_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod
