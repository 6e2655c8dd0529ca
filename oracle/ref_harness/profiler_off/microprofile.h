// profiler_off/microprofile.h — our own no-op stand-in for the profiler header the reference's .cpp files include
// (its src/microprofile is a submodule that the reference tree does not ship).  oracle/Makefile's `ref_full` puts this
// directory on the include path so that World.cpp, Solver.cpp, Collider.cpp and base/WorkQueue.cpp build unchanged.
//
// Why it cannot change a result: every macro below expands to nothing, so no argument is evaluated and no program state
// is read or written; the two thread hooks run only inside WorkQueue worker threads, and the harness always builds its
// queue with 0 workers (full_harness.cpp), so they are never even called.
#pragma once

#define MICROPROFILE_SCOPEI(...)
#define MICROPROFILE_SCOPEGPUI(...)
#define MICROPROFILE_COUNTER_SET(...)
#define MICROPROFILE_COUNTER_ADD(...)
#define MICROPROFILE_META_CPU(...)
#define MICROPROFILE_LABELF(...)

inline void MicroProfileOnThreadCreate(const char*) {}
inline void MicroProfileOnThreadExit() {}
