// Stand-alone host program for a sanitizer run of the native block reader (qcmrf_amd/csrc/ingest_native.cpp): an
// interpreter of its own with the reader compiled IN as a built-in module, so that the sanitized code is the code that
// runs (recipe: scripts/README.md).  Takes the command line of ``python``; run it on scripts/ingest_native_asan.py.
#include <Python.h>

extern "C" PyObject *PyInit__ingest_native(void);

int main(int argc, char **argv)
{
    if (PyImport_AppendInittab("_ingest_native", PyInit__ingest_native) < 0)
        return 2;
    return Py_BytesMain(argc, argv);
}
