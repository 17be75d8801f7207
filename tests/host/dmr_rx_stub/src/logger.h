// Stand-in for src/logger.h that counts what it is told, by level: the reference reports an embedded FLCO it does not know, and a burst that
// fails validate(), through its logger only.  Stands in front of tests/host/dmr_ctl_stub on the include path of tests/host/dmr_rx_ref.cpp.
#pragma once
#include <QString>
class Logger {
public:
    enum { LogLevelDebug, LogLevelInfo, LogLevelWarning, LogLevelCritical, LogLevelFatal };
    void log(int level, const QString&) { if (level >= 0 && level <= LogLevelFatal) ++count[level]; }
    unsigned count[LogLevelFatal + 1] = {};
};
