// Stand-alone host program for a sanitizer run of the native counts formatter (qcmrf_amd/csrc/counts_native.cpp): an
// interpreter of its own with the module compiled IN as a built-in, so that the sanitized code is the code that runs
// (recipe: scripts/README.md).  Takes the command line of ``python``; run it on scripts/counts_native_asan.py.
#include <Python.h>

extern "C" PyObject *PyInit__counts_native(void);

int main(int argc, char **argv)
{
    if (PyImport_AppendInittab("_counts_native", PyInit__counts_native) < 0)
        return 2;
    return Py_BytesMain(argc, argv);
}
