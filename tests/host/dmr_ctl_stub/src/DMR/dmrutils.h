// Stand-in for src/DMR/dmrutils.h: the two text conversions of DMRControl's talker-alias receive path, which no test here runs
#pragma once
#include <QSysInfo>
#include <QString>
class DMRUtils {
public:
    static void parseUTF16(QString&, unsigned int, unsigned char*) {}
    static void parseISO7bitToISO8bit(unsigned char*, unsigned char*, unsigned int, unsigned int) {}
};
