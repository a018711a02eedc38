"""What the wrappers of the C++ test programs (tests/cpp/*.cpp) share: where a program is, and the
make target that builds all of them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def binary(name):
    return os.path.join(ROOT, "tests", "cpp", name)


def build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "gpu-fhe_amd"), "cpptest"], check=True)
