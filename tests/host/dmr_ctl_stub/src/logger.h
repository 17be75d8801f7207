// Stand-in for src/logger.h: log() drops its text
#pragma once
#include <QString>
class Logger {
public:
    enum { LogLevelDebug, LogLevelInfo, LogLevelWarning, LogLevelCritical, LogLevelFatal };
    void log(int, const QString&) {}
};
