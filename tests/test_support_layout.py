"""The layout of tests/ itself: test modules use the support modules beside them (README.md,
"Tests") and never each other, support modules hold no tests, and one module alone knows where
bin/rt_render is.  Reads the files as text (no GPU, milliseconds)."""
import glob
import os
import re

TESTS = os.path.dirname(os.path.abspath(__file__))


def sources(test_modules):
    for path in sorted(glob.glob(os.path.join(TESTS, "*.py"))):
        name = os.path.basename(path)
        if name.startswith("test_") == test_modules:
            yield name, open(path).read()


def test_no_test_module_imports_another():
    # a changed test file cannot break the collection of another; at any indentation, so
    # that an import inside a function does not slip through
    found = {name: m for name, text in sources(True)
             if (m := re.findall(r"^[ \t]*(?:from|import)[ \t]+test_\w+", text, flags=re.M))}
    assert not found, found


def test_support_modules_hold_no_tests():
    found = {name: m for name, text in sources(False)
             if (m := re.findall(r"^[ \t]*def[ \t]+(test_\w*)", text, flags=re.M))}
    assert not found, found


def test_one_module_knows_the_path_of_rt_render():
    # the binary's name as a string among the arguments of a path join
    joined = re.compile(r"""join\([^()]*["']rt_render["']""")
    found = [name for test_modules in (True, False) for name, text in sources(test_modules) if joined.search(text)]
    assert found == ["driver.py"], found
